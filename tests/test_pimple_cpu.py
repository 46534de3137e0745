"""CPU tier of DAPimpleFoam: the numpy restatement (tests/pimple_residual.py) on its own, body_cell with the DDT flag and the hand-written
old-time product body_drdwold run on the host (tests/hostemu/hostemu_pimple.cpp) against it, the refusals by name and the time operators.
Bounds (tests/README_actuator_disk.md): values 1e-12 relative to the block's maximum, tangents and products 1e-10 against the complex step
of the restatement; "bitwise" is np.array_equal."""
import copy
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import actuator_disk_cases as ADC
from dafoam_amd import _capi
from dafoam_amd._capi import CaseStruct, das_case_t, dptr
from dafoam_amd.meshgen import channel_case, periodic_channel_case, pimple_case, simple_T_channel_case, turbo_channel_case
from dafoam_amd.pyDASolvers import pyDASolvers
from oracle.foam_mesh import Geometry
from oracle.residual import simple_residual
from pimple_cases import DELTA_T, MESHES, NORM, SCHEMES, blocks, geom, old_states, options, pimple_case_of, rel, scales, steady_case
from pimple_residual import ddt_coeffs, pimple_residual

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
dp = _capi.c_double_p
UNNORMALISED = ("TRes",)


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    """tests/hostemu/hostemu_pimple.cpp through g++, as the other harnesses are built; and the harness of the residual as it stands
    (tests/hostemu/hostemu.cpp), for the bitwise comparison."""
    rocm = os.environ.get("ROCM_PATH") or os.path.dirname(os.path.dirname(os.path.realpath(shutil.which("hipcc") or "/opt/rocm/bin/hipcc")))
    d = tmp_path_factory.mktemp("hostemu")
    libs = []
    for src in ("hostemu_pimple.cpp", "hostemu.cpp"):
        so = str(d / ("lib" + src.replace(".cpp", ".so")))
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fopenmp", "-fPIC", "-shared", "-I" + os.path.join(rocm, "include"), "-D__HIP_PLATFORM_AMD__",
                               "-o", so, os.path.join(ROOT, "tests", "hostemu", src), os.path.join(ROOT, "dafoam_amd", "csrc", "das_mesh.cpp")])
        libs.append(C.CDLL(so))
    L, L.plain = libs
    L.emu_pimple_residual.argtypes = [C.POINTER(das_case_t), dp, C.c_longlong, dp, dp, C.c_int, C.c_int, C.c_double, C.c_int, dp, dp, dp, dp]
    L.emu_pimple_drdwold.argtypes = [C.POINTER(das_case_t), dp, C.c_longlong, dp, dp, C.c_int, C.c_int, C.c_int, dp, dp, dp]
    L.plain.emu_residual.argtypes = [C.POINTER(das_case_t), dp, C.c_longlong, C.c_int, dp, dp, dp]
    L.plain.emu_set_pc_blend.argtypes = [C.c_double]
    return L


def arr(a):
    return None if a is None else dptr(np.ascontiguousarray(a, dtype=np.float64))


def emu_residual(L, case, W, W0, W00, ti, isPC=0, blend=0.0, normalized=1, dW0=None, dW00=None):
    R, Rd = np.zeros(W.size), np.zeros(W.size)
    keep = [np.ascontiguousarray(a, dtype=np.float64) if a is not None else None for a in (W, W0, W00, dW0, dW00)]
    assert L.emu_pimple_residual(CaseStruct(case).byref(), arr(keep[0]), W.size, arr(keep[1]), arr(keep[2]), ti, isPC, blend, normalized, arr(keep[3]), arr(keep[4]),
                                 dptr(R), dptr(Rd)) == 0
    return R, Rd


def emu_product(L, case, W, W0, W00, ti, level, psi, scale, normalized=1):
    out = np.zeros(W.size)
    keep = [np.ascontiguousarray(a, dtype=np.float64) for a in (W, W0, W00, scale, psi)]
    assert L.emu_pimple_drdwold(CaseStruct(case).byref(), dptr(keep[0]), W.size, dptr(keep[1]), dptr(keep[2]), ti, level, normalized, dptr(keep[3]), dptr(keep[4]),
                                dptr(out)) == 0
    return out


def product_by_complex_step(case, g, W, W0, W00, ti, level, psi, scale, cols, **kw):
    """scale_j psi . dR/dW0_j (level 1) or dW00_j (level 2) at the columns cols: one complex step of the restatement per column"""
    out = np.zeros(len(cols))
    for i, j in enumerate(cols):
        e = np.zeros(W.size, dtype=complex)
        e[j] = 1e-30j
        R = pimple_residual(case, g, W, W0 + e if level == 1 else W0, W00 + e if level == 2 else W00, time_index=ti, **kw)
        out[i] = scale[j] * float(psi @ (np.imag(R) / 1e-30))
    return out


# ---- the restatement on its own -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mesh", ADC.MESHES)
def test_restatement_without_ddt_has_the_bits_of_the_oracle(mesh):
    case = ADC.disk_case(mesh)
    go, W = Geometry(case.mesh), case.states
    for kw in (dict(), dict(normalize=UNNORMALISED), dict(isPC=True)):
        assert np.array_equal(simple_residual(case, go, W, **kw), pimple_residual(case, go, W, W, W, coeffs=(0.0, 0.0, 0.0), relax_U=None, **kw))


@pytest.mark.parametrize("mesh", MESHES)
def test_restatement_time_derivative_vanishes_at_W0_equal_W(mesh):
    """W0 = W under Euler, relax_U = 1 on the case: the U and nuTilda rows are the steady ones to rounding - (c V / dt) x and (V / dt) x0
    cancel in M & x - source.  The p and phi rows are NOT the steady ones and no restatement can make them so: c / dt stays in A, and
    HbyA = H / A with it (pRes = div(rAU grad p) - div(HbyA) agrees with the steady row only where URes = 0); the difference is printed."""
    g, W = geom(mesh), steady_case(mesh).states
    steady = copy.copy(steady_case(mesh))
    steady.relax = dict(steady.relax, U=1.0)
    R0 = simple_residual(steady, g, W)
    R = pimple_residual(pimple_case_of(mesh), g, W, W, None, time_index=1)
    b = blocks(g)
    errs = {k: rel(R[sl], R0[sl]) for k, sl in b.items()}
    print(mesh, errs)
    # rounding: eps times the cancelled term x / dt over the block's maximum
    for k in ("U", "nuTilda"):
        assert errs[k] <= 1e-12
    assert errs["p"] > 1e-6 and errs["phi"] > 1e-6


def test_ddt_coefficients():
    assert ddt_coeffs("Euler", 1) == ddt_coeffs("Euler", 5) == ddt_coeffs("backward", 1) == (1.0, 1.0, 0.0)
    assert ddt_coeffs("backward", 2) == ddt_coeffs("backward", 3) == (1.5, 2.0, 0.5)
    with pytest.raises(ValueError, match="CrankNicolson not supported"):
        ddt_coeffs("CrankNicolson", 1)


# ---- body_cell with the DDT flag on the host ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("mesh", MESHES)
@pytest.mark.parametrize("scheme,ti", SCHEMES)
def test_hostemu_residual(emu, mesh, scheme, ti):
    case, g = pimple_case_of(mesh, scheme), geom(mesh)
    W = steady_case(mesh).states
    W0, W00 = old_states(mesh)
    for label, ekw, rkw in (("normalised", dict(), dict()), ("not normalised", dict(normalized=0), dict(normalize=UNNORMALISED)),
                            ("PC, blend 0.5", dict(isPC=1, blend=0.5), dict(isPC=True, pc_blend=0.5))):
        R, _ = emu_residual(emu, case, W, W0, W00, ti, **ekw)
        ref = pimple_residual(case, g, W, W0, W00, time_index=ti, **rkw)
        errs = {k: rel(R[sl], ref[sl]) for k, sl in blocks(g).items()}
        print(mesh, scheme, ti, label, errs)
        assert max(errs.values()) <= 1e-12
    if (scheme, ti) == ("backward", 1):  # exactly Euler: the same bits, whatever W00 holds
        Re, _ = emu_residual(emu, pimple_case_of(mesh, "Euler"), W, W0, None, 1)
        Rb, _ = emu_residual(emu, case, W, W0, W00, 1)
        assert np.array_equal(Re, Rb)
    if (scheme, ti) == ("backward", 3):  # and both old levels are live
        Rb1, _ = emu_residual(emu, case, W, W0, W00, 1)
        Rb3, _ = emu_residual(emu, case, W, W0, W00, 3)
        Rb3b, _ = emu_residual(emu, case, W, W0, W0, 3)
        assert not np.array_equal(Rb1, Rb3) and not np.array_equal(Rb3, Rb3b)


@pytest.mark.parametrize("mesh", MESHES)
def test_hostemu_flag_off_is_the_harness_as_it_stands(emu, mesh):
    case = steady_case(mesh)
    W = np.ascontiguousarray(case.states)
    cs = CaseStruct(case)
    for isPC, blend in ((0, 0.0), (1, 0.5)):
        R, _ = emu_residual(emu, case, W, None, None, 1, isPC=isPC, blend=blend)
        Rp = np.zeros(W.size)
        emu.plain.emu_set_pc_blend(blend)
        try:
            assert emu.plain.emu_residual(cs.byref(), dptr(W), W.size, isPC, None, dptr(Rp), None) == 0
        finally:
            emu.plain.emu_set_pc_blend(0.0)
        assert np.array_equal(R, Rp)


# ---- the old-time product on the host -------------------------------------------------------------------------------------------------
def product_columns(g, rng):
    """the U, p and nuTilda states of three cells, a face, and six random ones"""
    N = g.nC
    cells = (0, N // 2, N - 1)
    cols = [3 * c + k for c in cells for k in range(3)] + [3 * N + c for c in cells] + [4 * N + c for c in cells] + [5 * N + g.nIF // 2]
    return np.array(cols + list(rng.integers(0, 5 * N + g.nF, 6)))


@pytest.mark.parametrize("mesh", MESHES)
@pytest.mark.parametrize("scheme,ti", SCHEMES)
def test_hostemu_old_time_product(emu, mesh, scheme, ti):
    case, g = pimple_case_of(mesh, scheme), geom(mesh)
    W = steady_case(mesh).states
    W0, W00 = old_states(mesh)
    rng = np.random.default_rng(5)
    psi = rng.standard_normal(W.size)
    cols = np.arange(W.size) if mesh == "small" else product_columns(g, rng)
    for norm_states in (NORM, None):
        s = scales(g, norm_states)
        for normalized, rkw in ((1, dict()), (0, dict(normalize=UNNORMALISED))):
            for level in (1, 2):
                out = emu_product(emu, case, W, W0, W00, ti, level, psi, s, normalized)
                c00 = ddt_coeffs(scheme, ti)[2]
                if level == 2 and c00 == 0.0:
                    assert not out.any()
                    continue
                ref = product_by_complex_step(case, g, W, W0, W00, ti, level, psi, s, cols, **rkw)
                err = rel(out[cols], ref)
                print(mesh, scheme, ti, "states scaled" if norm_states else "states plain", "normalised" if normalized else "not normalised", "level", level, err)
                assert np.abs(ref).max() > 0 and err <= 1e-10
                b = blocks(g)
                assert not out[b["p"]].any() and not out[b["phi"]].any()


@pytest.mark.parametrize("mesh", MESHES)
def test_hostemu_old_time_product_dot_identity(emu, mesh):
    """psi . (dR/dW0 v) = v . (dR/dW0^T psi): the left side from one dual pass with tangents on W0 (W00), a pass of the harness only"""
    case, g = pimple_case_of(mesh, "backward"), geom(mesh)
    W = steady_case(mesh).states
    W0, W00 = old_states(mesh)
    rng = np.random.default_rng(6)
    psi, v = rng.standard_normal(W.size), rng.standard_normal(W.size)
    ones = np.ones(W.size)
    for level in (1, 2):
        _, Rd = emu_residual(emu, case, W, W0, W00, 3, dW0=v if level == 1 else None, dW00=v if level == 2 else None)
        left, right = float(psi @ Rd), float(v @ emu_product(emu, case, W, W0, W00, 3, level, psi, ones))
        print(mesh, "level", level, left, right)
        assert abs(left - right) <= 1e-10 * abs(left)


@pytest.mark.parametrize("mesh", MESHES)
def test_old_time_product_needs_the_H_part(emu, mesh):
    """Seeds on the p and phi rows only: the U0 entries come through HbyA -> phiHbyA alone.  A product that keeps the diagonal gives zeros
    there: its miss is the whole entry (measured: relative error 1.0 on every mesh, against the bound 1e-10)."""
    case, g = pimple_case_of(mesh, "backward"), geom(mesh)
    W = steady_case(mesh).states
    W0, W00 = old_states(mesh)
    b = blocks(g)
    rng = np.random.default_rng(7)
    psi = rng.standard_normal(W.size)
    psi[b["U"]] = 0.0
    psi[b["nuTilda"]] = 0.0
    s = scales(g)
    cols = np.arange(3 * g.nC) if mesh == "small" else product_columns(g, rng)[:9]
    for level in (1, 2):
        out = emu_product(emu, case, W, W0, W00, 3, level, psi, s)
        ref = product_by_complex_step(case, g, W, W0, W00, 3, level, psi, s, cols)
        c0 = (2.0, -0.5)[level - 1]
        diagonal_only = -c0 / DELTA_T * s * psi  # what a diagonal scaling of psi would give: zeros in the U0 entries here
        print(mesh, "level", level, "H part", rel(out[cols], ref), "diagonal only", rel(diagonal_only[cols], ref))
        assert np.abs(out[b["U"]]).min() > 0 and rel(out[cols], ref) <= 1e-10
        assert rel(diagonal_only[cols], ref) == 1.0


# ---- refusals by name -------------------------------------------------------------------------------------------------------------------
def as_pimple(case, **kw):
    case = copy.copy(case)
    case.solver_name, case.ddt_scheme, case.deltaT, case.n_steps = "DAPimpleFoam", "Euler", DELTA_T, 6
    for k, v in kw.items():
        setattr(case, k, v)
    return case


def test_refusals_by_name():
    base = pimple_case_of("small")
    with pytest.raises(_capi.DASError, match="ddtScheme CrankNicolson not supported! Options: steadyState, Euler, or backward"):
        pyDASolvers("DAPimpleFoam -python", options(), case=as_pimple(base, ddt_scheme="CrankNicolson"))
    with pytest.raises(_capi.DASError, match="DAPimpleFoam: the T field is not built"):
        pyDASolvers("DAPimpleFoam -python", options(), case=as_pimple(simple_T_channel_case(5, 4, 3)))
    with pytest.raises(_capi.DASError, match="DAPimpleFoam: MRF is not built"):
        pyDASolvers("DAPimpleFoam -python", options(), case=as_pimple(base, mrf={"omega": (10.0, 0.0, 0.0), "origin": (0.0, 0.0, 0.0)}))
    with pytest.raises(_capi.DASError, match="DAPimpleFoam: cyclic patches are not built"):
        pyDASolvers("DAPimpleFoam -python", options(), case=as_pimple(periodic_channel_case(5, 4, 3)))
    with pytest.raises(_capi.DASError, match="DAPimpleFoam: simple_consistent is not built"):
        pyDASolvers("DAPimpleFoam -python", options(), case=as_pimple(base, simple_consistent=True))
    with pytest.raises(_capi.DASError, match=r"fvSource\[disk\]: the fvSource option is not built for DAPimpleFoam"):
        pyDASolvers("DAPimpleFoam -python", options(fvSource={"disk": dict(ADC.DISK_A)}), case=base)
    with pytest.raises(_capi.DASError, match="regressionModel: the option is not built for DAPimpleFoam"):
        pyDASolvers("DAPimpleFoam -python", options(regressionModel={"active": True, "model1": {}}), case=base)
    with pytest.raises(_capi.DASError, match=r"outputInfo\[f\]: coupling outputs are not built for DAPimpleFoam"):
        pyDASolvers("DAPimpleFoam -python", options(outputInfo={"f": {"type": "forceCouplingOutput", "patches": ["bottom"], "components": ["forceCoupling"], "pRef": 0.0}}), case=base)
    with pytest.raises(_capi.DASError, match=r"inputInfo\[t\]: coupling inputs \(thermalCoupling\) are not built for DAPimpleFoam"):
        pyDASolvers("DAPimpleFoam -python", options(inputInfo={"t": {"type": "thermalCoupling", "patches": ["bottom"], "components": ["solver"]}}), case=base)
    with pytest.raises(_capi.DASError, match="DAPimpleFoam: dynamicMesh is not built"):
        pyDASolvers("DAPimpleFoam -python", options(dynamicMesh={"active": True}), case=base)
    with pytest.raises(_capi.DASError, match="adjEqnSolMethod fixedPoint is not built"):
        pyDASolvers("DAPimpleFoam -python", options(adjEqnSolMethod="fixedPoint"), case=base)
    with pytest.raises(_capi.DASError, match="function q: type meshQualityKS is not built for DAPimpleFoam"):
        pyDASolvers("DAPimpleFoam -python", options(function={"q": {"type": "meshQualityKS", "coeffKS": 10.0, "metric": "nonOrthoAngle"}}), case=base)
    with pytest.raises(_capi.DASError, match="function f: timeOp max is not built for DAPimpleFoam"):
        pyDASolvers("DAPimpleFoam -python", options(function={"f": {"type": "force", "patches": ["bottom"], "direction": [1.0, 0.0, 0.0], "timeOp": "max"}}), case=base)
    s = pyDASolvers("DAPimpleFoam -python", options(), case=base)
    with pytest.raises(_capi.DASError, match="DAPimpleFoam: simpleIteration is not built"):
        s.simpleIteration(1)
    with pytest.raises(AttributeError, match="runFPAdj"):  # the fixed-point adjoint is a method no solver of this path has
        s.runFPAdj()
    # the library's own entry refuses what would reach it without the Python layer
    for kw, msg in ((dict(has_T=True), "T field"), (dict(mrf={"omega": (1.0, 0.0, 0.0)}), "MRF")):
        c = as_pimple(simple_T_channel_case(5, 4, 3) if "has_T" in kw else base, **kw)
        assert not _capi.lib().das_create(CaseStruct(c).byref())
        assert msg in _capi.lib().das_last_error().decode()
    # old-time states exist for this solver alone, and the backward scheme needs both levels from the second step on
    steady = pyDASolvers("DASimpleFoam -python", dict(options(), solverName="DASimpleFoam"), case=steady_case("small"))
    with pytest.raises(_capi.DASError, match="old-time states only exist for DAPimpleFoam"):
        steady.setOldTimeStates(base.states)
    assert steady.getDdtSchemeOrder() == 1 and s.getDdtSchemeOrder() == 1
    sb = pyDASolvers("DAPimpleFoam -python", options(), case=pimple_case_of("small", "backward"))
    assert sb.getDdtSchemeOrder() == 2
    with pytest.raises(_capi.DASError, match="the backward scheme at time index 2 needs W00"):
        sb.setOldTimeStates(base.states, None, 2)


def test_sharded_solvers_and_case_directories_are_refused(tmp_path):
    from dafoam_amd import distributed, foam_io

    with pytest.raises(NotImplementedError, match="sharded \\(multi-rank\\) DAPimpleFoam solvers are not built"):
        distributed.extract_submesh(pimple_case_of("small"), np.zeros(pimple_case_of("small").mesh.n_cells, dtype=np.int64), 0)
    # foam_io stays as it is: it verifies system/fvSchemes against the implemented (steady) scheme set, so the directory of such a case is
    # refused with the offending entry named
    d = str(tmp_path / "case")
    foam_io.write_case(d, steady_case("small"))
    p = os.path.join(d, "system", "fvSchemes")
    text = open(p).read()
    assert "default steadyState" in text
    open(p, "w").write(text.replace("default steadyState", "default Euler"))
    with pytest.raises(NotImplementedError, match=r"system/fvSchemes asks for schemes the GPU kernels do not implement .*ddtSchemes.*Euler"):
        foam_io.read_case(d, solver_name="DAPimpleFoam")


# ---- the time operators ---------------------------------------------------------------------------------------------------------------
def test_time_operator_scalings():
    """DATimeOpAverage.C / DATimeOpFinal.C with getTimeOpRange (DASolver.C:404-422) for 6 steps: average - 1 / window inside the trailing
    window max(2, round(nStepsFrac 6)), 0 before it, the window's mean; final - the last value, scaling 1 at the last step and 0 before
    it: the derivative of what DATimeOpFinal::compute returns (its dFScaling returns 1 at every index - the derivative of the sum over
    the steps, which central differences of the marched primal refute, tests/README_pimple.md)."""
    fn = lambda **kw: dict({"type": "force", "patches": ["bottom"], "direction": [1.0, 0.0, 0.0]}, **kw)
    s = pyDASolvers("DAPimpleFoam -python", options(function={"final": fn(timeOp="final"), "all": fn(timeOp="average", nStepsFrac=1.0),
                                                               "half": fn(timeOp="average", nStepsFrac=0.5), "default": fn(timeOp="average"),
                                                               "plain": fn()}), case=pimple_case_of("small"))
    vals = [3.0, 1.0, 4.0, 1.0, 5.0, 9.0]
    s._functionTimeSteps = {k: list(vals) for k in ("final", "all", "half", "default", "plain")}
    idx = range(6)
    assert [s.getdFScaling("final", i) for i in idx] == [0.0] * 5 + [1.0] and [s.getdFScaling("plain", i) for i in idx] == [0.0] * 5 + [1.0]
    assert [s.getdFScaling("all", i) for i in idx] == [1.0 / 6] * 6
    assert [s.getdFScaling("half", i) for i in idx] == [0.0] * 3 + [1.0 / 3] * 3
    assert [s.getdFScaling("default", i) for i in idx] == [0.0] * 4 + [0.5] * 2  # round(0.2 x 6) = 1 -> the floor of 2 steps
    assert s.getdFScaling("final", 6) == 0.0 and s.getdFScaling("all", -1) == 0.0
    assert s.getTimeOpFuncVal("final") == 9.0 == s.getTimeOpFuncVal("plain")
    assert s.getTimeOpFuncVal("all") == sum(vals) / 6 and s.getTimeOpFuncVal("half") == (1.0 + 5.0 + 9.0) / 3 and s.getTimeOpFuncVal("default") == 7.0
    with pytest.raises(_capi.DASError, match="functionName nope not found"):
        s.getdFScaling("nope", 0)


def test_pimple_case_is_the_channel_with_the_time_settings():
    a, b = channel_case(6, 5, 4), pimple_case(6, 5, 4, ddt_scheme="backward", deltaT=0.02, n_steps=4)
    assert (b.solver_name, b.ddt_scheme, b.deltaT, b.n_steps) == ("DAPimpleFoam", "backward", 0.02, 4)
    assert np.array_equal(a.states, b.states) and np.array_equal(a.mesh.points, b.mesh.points) and a.bcs == b.bcs
