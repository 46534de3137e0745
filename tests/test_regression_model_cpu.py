"""CPU tier of the regression models (the regressionModel option and the regressionPar input of DASimpleFoam): the DAS_HD bodies of
csrc/das_regression.hpp run on the host (tests/hostemu/hostemu_regression.cpp) against the numpy restatement of the reference's text
(tests/regression_model_restatement.py), and the refusals that need no device, through Python and the C entries.
Bounds (tests/README_regression.md): values 1e-12, tangents and products 1e-10 relative to the largest entry, finite-difference checks
1e-6; counts and the zeros of clipped cells are exact."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import regression_model_restatement as RM
from dafoam_amd import _capi
from dafoam_amd._capi import dptr
from dafoam_amd.meshgen import channel_case, heat_transfer_case, rho_channel_case
from dafoam_amd.pyDASolvers import pyDASolvers
from mixed_mesh import mixed
from oracle.foam_mesh import Geometry

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
dp = _capi.c_double_p
ip = _capi.c_int_p
TYPES = {"neuralNetwork": 0, "radialBasisFunction": 1}
ACTS = {"sigmoid": 0, "tanh": 1, "relu": 2}


def rel(a, b):
    return float(np.abs(np.asarray(a) - np.asarray(b)).max() / max(np.abs(b).max(), 1e-300))


def specs(model, nInputs=None):
    """the flat description tests/hostemu/hostemu_regression.cpp takes"""
    names = model.get("inputNames") or []
    nIn = len(names) if nInputs is None else nInputs
    h = list(model.get("hiddenLayerNeurons", []))
    i = np.zeros(19, dtype=np.int32)
    i[:5] = [TYPES[model["modelType"]], nIn, len(h), model.get("nRBFs", 0), ACTS.get(model.get("activationFunction"), 0)]
    i[5:5 + len(names)] = [RM.FEATURES.index(n) for n in names]
    i[13:13 + len(h)] = h
    d = np.zeros(22)
    d[:nIn] = model["inputShift"][:nIn]
    d[8:8 + nIn] = model["inputScale"][:nIn]
    d[16:] = [model.get("leakyCoeff", 0.0), model["outputShift"], model["outputScale"], model["outputUpperBound"], model["outputLowerBound"],
              model["defaultOutputValue"]]
    return i, d


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    rocm = os.environ.get("ROCM_PATH") or os.path.dirname(os.path.dirname(os.path.realpath(shutil.which("hipcc") or "/opt/rocm/bin/hipcc")))
    so = str(tmp_path_factory.mktemp("hostemu") / "libhostemu_regression.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fopenmp", "-fPIC", "-shared", "-I" + os.path.join(rocm, "include"), "-D__HIP_PLATFORM_AMD__", "-o", so,
                           os.path.join(ROOT, "tests", "hostemu", "hostemu_regression.cpp"), os.path.join(ROOT, "dafoam_amd", "csrc", "das_mesh.cpp")])
    L = C.CDLL(so)
    ub = C.POINTER(C.c_ubyte)
    L.emu_reg_n_parameters.argtypes = [ip, dp]
    L.emu_reg_features.argtypes = [ip, dp, C.c_int, C.c_double] + [dp] * 11
    L.emu_reg_forward.argtypes = [ip, dp, dp, C.c_int, dp, dp, C.c_int, dp, dp, ub]
    L.emu_reg_backward.argtypes = [ip, dp, dp, C.c_int, dp, dp, dp]
    return L


def arr(a):
    return None if a is None else dptr(np.ascontiguousarray(a, dtype=np.float64).ravel())


def emu_forward(L, model, par, feat, dfeat=None, seed=0, dual=False):
    i, d = specs(model)
    n = feat.shape[0]
    b, db, m = np.zeros(n), np.zeros(n), np.zeros(n, dtype=np.uint8)
    want_dual = dual or dfeat is not None or seed
    assert L.emu_reg_forward(i.ctypes.data_as(ip), dptr(d), arr(par), n, arr(feat), arr(dfeat), seed, dptr(b), dptr(db) if want_dual else None,
                             m.ctypes.data_as(C.POINTER(C.c_ubyte))) == 0
    return b, db, m.astype(np.int64)


def emu_backward(L, model, par, feat, g):
    i, d = specs(model)
    out = np.zeros(len(par))
    assert L.emu_reg_backward(i.ctypes.data_as(ip), dptr(d), arr(par), feat.shape[0], arr(feat), arr(g), dptr(out)) == 0
    return out


@pytest.fixture(scope="module", params=["channel", "mixed"])
def flow(request):
    """states with a non-zero gradient everywhere on the 6 x 5 x 4 channel and on the 148-cell mixed mesh, and the oracle's gradients"""
    case = channel_case(6, 5, 4) if request.param == "channel" else mixed("simple")
    g = Geometry(case.mesh)
    W = RM.stirred_states(case)
    U, nuT, gradU, gradP, y = RM.flow_inputs(case, g, W)
    assert np.abs(gradU).reshape(g.nC, 9).max(1).min() > 0 and np.abs(gradP).max(1).min() > 0
    return dict(case=case, g=g, W=W, U=U, nuT=nuT, gradU=gradU, gradP=gradP, y=y, nu=case.nu)


ALL7 = RM._model(modelType="neuralNetwork", inputNames=list(RM.FEATURES), hiddenLayerNeurons=[3], activationFunction="sigmoid")


def model_features(f, model):
    return RM.features(model, f["U"], f["nuT"], f["nu"], f["gradU"], f["gradP"], f["y"])


# ---- 1: the seven features ---------------------------------------------------------------------------------------------------------------
def test_each_feature_against_the_restatement(emu, flow):
    f = flow
    ref = model_features(f, ALL7)
    i, d = specs(ALL7)
    out = np.zeros_like(ref)
    assert emu.emu_reg_features(i.ctypes.data_as(ip), dptr(d), f["g"].nC, f["nu"], arr(f["U"]), arr(f["nuT"]), arr(f["gradU"]), arr(f["gradP"]), arr(f["y"]), None,
                                None, None, None, dptr(out), None) == 0
    for k, name in enumerate(RM.FEATURES):
        e = np.abs(out[:, k] - ref[:, k]).max()
        print(name, "range", ref[:, k].min(), ref[:, k].max(), "err", e)
        assert np.ptp(ref[:, k]) > 1e-3  # the feature is live on these states
        assert e <= 1e-12


def test_feature_tangents_against_central_differences_of_the_restatement(emu, flow):
    f = flow
    rng = np.random.default_rng(3)
    N = f["g"].nC
    dU, dN, dgU, dgP = rng.standard_normal((N, 3)), 1e-4 * rng.standard_normal(N), rng.standard_normal((N, 3, 3)), rng.standard_normal((N, 3))
    i, d = specs(ALL7)
    out, dout = np.zeros((N, 7)), np.zeros((N, 7))
    assert emu.emu_reg_features(i.ctypes.data_as(ip), dptr(d), N, f["nu"], arr(f["U"]), arr(f["nuT"]), arr(f["gradU"]), arr(f["gradP"]), arr(f["y"]), arr(dU),
                                arr(dN), arr(dgU), arr(dgP), dptr(out), dptr(dout)) == 0
    L_ = np.longdouble
    h = L_(1e-7)
    at = lambda s: RM.features(ALL7, f["U"].astype(L_) + s * h * dU, f["nuT"].astype(L_) + s * h * dN, f["nu"], f["gradU"].astype(L_) + s * h * dgU,
                               f["gradP"].astype(L_) + s * h * dgP, f["y"].astype(L_))
    fd = ((at(1) - at(-1)) / (2 * h)).astype(np.float64)
    for k, name in enumerate(RM.FEATURES):
        print(name, "tangent err", rel(dout[:, k], fd[:, k]))
        assert rel(dout[:, k], fd[:, k]) <= 1e-6


def test_mag_of_an_exactly_zero_vector_is_zero_with_a_zero_tangent(emu):
    """the dsqrt convention of das_dual.hpp: a cell at rest with no gradient gives finite features and finite (zero) tangents, no NaN"""
    i, d = specs(ALL7)
    z3, z9, one = np.zeros(3), np.zeros(9), np.ones(1)
    out, dout = np.zeros(7), np.zeros(7)
    assert emu.emu_reg_features(i.ctypes.data_as(ip), dptr(d), 1, 1.5e-5, arr(z3), arr(1e-4 * one), arr(z9), arr(z3), arr(0.01 * one), arr(np.ones(3)),
                                arr(one), arr(np.ones(9)), arr(np.ones(3)), dptr(out), dptr(dout)) == 0
    assert np.isfinite(out).all() and np.isfinite(dout).all()
    k = RM.FEATURES.index("VoS")
    assert out[k] == (0.0 + ALL7["inputShift"][k]) * ALL7["inputScale"][k] and dout[k] == 0.0


# ---- 2: forward values -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["nn3", "nn534", "nn2020", "rbf1", "rbf7"])
def test_forward_values_against_the_restatement(emu, flow, name):
    model = RM.MODELS[name]
    par = RM.parameters(model)
    feat = model_features(flow, model)
    ref, mask = RM.beta(model, par, feat)
    b, _, m = emu_forward(emu, model, par, feat)
    print(name, "beta range", ref.min(), ref.max(), "err", np.abs(b - ref).max())
    assert np.ptp(ref) > 1e-3 and not mask.any() and not m.any()
    assert np.abs(b - ref).max() <= 1e-12 * max(1.0, np.abs(ref).max())


def test_forward_tangent_against_central_differences(emu, flow):
    for name in ("nn534", "nn2020", "rbf7"):
        model = RM.MODELS[name]
        par = RM.parameters(model)
        feat = model_features(flow, model)[:20]
        dfeat = np.random.default_rng(5).standard_normal(feat.shape)
        _, db, _ = emu_forward(emu, model, par, feat, dfeat=dfeat)
        L_ = np.longdouble
        h = L_(1e-7)
        fd = ((RM.beta(model, par.astype(L_), feat.astype(L_) + h * dfeat)[0] - RM.beta(model, par.astype(L_), feat.astype(L_) - h * dfeat)[0]) / (2 * h))
        print(name, "tangent err", rel(db, fd.astype(np.float64)))
        assert rel(db, fd.astype(np.float64)) <= 1e-6


# ---- 3: bounds -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["nn534", "rbf7"])
def test_bounds_counts_exact_and_zero_tangents_on_clipped_cells(emu, flow, name):
    base = RM.MODELS[name]
    par = RM.parameters(base)
    feat = model_features(flow, base)
    raw = RM.raw_output(base, par, feat)
    lo, hi = np.quantile(raw, 0.25), np.quantile(raw, 0.7)
    model = RM.clipped(base, lo, hi)
    ref, mask = RM.beta(model, par, feat)
    nClip = int((mask != 0).sum())
    print(name, "clipped", nClip, "of", mask.size, "below", int((raw < lo).sum()), "above", int((raw > hi).sum()))
    assert 0 < (raw < lo).sum() and 0 < (raw > hi).sum() and nClip < mask.size - 10  # checked on the restatement: some clip on each side, many do not
    dfeat = np.ones_like(feat)
    b, db, m = emu_forward(emu, model, par, feat, dfeat=dfeat)
    assert np.array_equal(m, mask) and RM.fail_counts(m) == RM.fail_counts(mask) == [0, 0, nClip]
    assert np.abs(b - ref).max() <= 1e-12
    assert np.all(db[mask != 0] == 0.0) and np.all(db[mask == 0] != 0.0)
    # the seeded pass of the regressionPar product: 1 after the bounds where the value stands, 0 on the clipped cells
    _, ds, _ = emu_forward(emu, model, par, feat, seed=1)
    assert np.array_equal(ds, (mask == 0).astype(float))


def test_nan_and_inf_are_replaced_and_counted(emu):
    model = dict(RM.MODELS["rbf1"], defaultOutputValue=0.75, outputLowerBound=0.0, outputUpperBound=2.0)
    par = RM.parameters(model)
    feat = np.array([[0.1, 0.2, 0.3], [np.nan, 0.2, 0.3], [0.3, 0.1, 0.2]])
    ref, mask = RM.beta(model, par, feat)
    b, db, m = emu_forward(emu, model, par, feat, dfeat=np.ones_like(feat))
    assert RM.fail_counts(mask) == [1, 0, 0] and np.array_equal(m, mask) and b[1] == 0.75 and db[1] == 0.0
    assert np.abs(b - ref).max() <= 1e-12 and db[0] != 0.0 and db[2] != 0.0
    # an infinite output: a weight of 1e308 twice over
    big = dict(RM.MODELS["nn3"], activationFunction="relu", outputScale=1e308, defaultOutputValue=0.5)
    pb = np.full(RM.n_parameters(big), 1e3)
    fb = np.full((2, 4), 1e3)
    refb, maskb = RM.beta(big, pb, fb)
    bb, _, mb = emu_forward(emu, big, pb, fb)
    assert RM.fail_counts(maskb) == [0, 2, 0] and np.array_equal(mb, maskb) and np.all(bb == 0.5) and np.array_equal(bb, refb)


# ---- 4: the backward body --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,cells", [("nn3", 40), ("nn534", 40), ("nn2020", 6), ("rbf1", 40), ("rbf7", 40)])
def test_backward_against_central_differences_of_the_restatement(emu, flow, name, cells):
    model = RM.MODELS[name]
    par = RM.parameters(model)
    feat = model_features(flow, model)[:cells]
    g = np.random.default_rng(11).standard_normal(cells)
    out = emu_backward(emu, model, par, feat, g)
    fd = RM.dbeta_dpar_fd(model, par, feat, g)
    print(name, len(par), "parameters, err", rel(out, fd), "smallest |entry| / largest", np.abs(fd).min() / np.abs(fd).max())
    assert rel(out, fd) <= 1e-6


def test_backward_with_clipped_cells(emu, flow):
    base = RM.MODELS["nn534"]
    par = RM.parameters(base)
    feat = model_features(flow, base)[:40]
    raw = RM.raw_output(base, par, feat)
    model = RM.clipped(base, np.quantile(raw, 0.3), np.quantile(raw, 0.7))
    _, mask = RM.beta(model, par, feat)
    assert 0 < (mask != 0).sum() < 40
    g = np.random.default_rng(12).standard_normal(40)
    out = emu_backward(emu, model, par, feat, g * (mask == 0))  # the seeded dual pass leaves g zero on the clipped cells
    assert rel(out, RM.dbeta_dpar_fd(model, par, feat, g)) <= 1e-6


@pytest.mark.parametrize("name", ["nn534", "nn2020", "rbf7"])
def test_backward_skips_replaced_cells_with_nan_and_inf_features(emu, name):
    """a NaN and an Inf cell among good ones: checkOutput replaced them (or, for the radial basis functions, left a finite value), their g
    is zero, and the reverse pass contributes exactly nothing from them - no 0 x NaN reaches any parameter"""
    model = dict(RM.MODELS[name], defaultOutputValue=0.75)
    par = RM.parameters(model)
    rng = np.random.default_rng(5)
    n, nIn = 30, len(model["inputNames"])
    feat, g = rng.random((n, nIn)), rng.standard_normal(n)
    feat[3, 1], feat[20, 0] = np.nan, np.inf
    ref, mask = RM.beta(model, par, feat)
    b, ds, m = emu_forward(emu, model, par, feat, seed=1)
    assert np.array_equal(m, mask) and mask[3] != 0 and np.array_equal(ds, (mask == 0).astype(float))
    g = g * ds  # what the seeded dual pass hands over
    g[20] = 0.0  # (the RBF keeps the Inf cell: its output is finite; its terms are 0 x inf in the reference's tape as well - not under test)
    out = emu_backward(emu, model, par, feat, g)
    good = np.ones(n, dtype=bool)
    good[[3, 20]] = False
    out_good = emu_backward(emu, model, par, feat[good], g[good])
    assert np.isfinite(out).all() and np.array_equal(out, out_good) and np.abs(out_good).max() > 0


def test_lds_of_the_backward_kernel_is_a_cap_at_definition():
    """[32, 32, 32, 22, 22, 20] on one input: 3889 parameters, under DAS_REG_MAX_PARAMS, but 1 + 2 x 160 + 1 = 322 rows of 512 bytes in the
    backward kernel, over the 160 KB of a compute unit: refused when it is defined, by name; 20 -> 18 neurons (318 rows) is admitted"""
    one = dict(inputNames=["VoS"], inputShift=[0.0], inputScale=[1.0])
    with pytest.raises(_capi.DASError, match="DAS_REG_MAX_LDS") as e:
        solver(channel_case(4, 3, 3), regressionModel=reg(big=dict(RM.MODELS["nn3"], hiddenLayerNeurons=[32, 32, 32, 22, 22, 20], **one)))
    assert "big" in str(e.value) and "164864" in str(e.value)
    s = solver(channel_case(4, 3, 3), regressionModel=reg(big=dict(RM.MODELS["nn3"], hiddenLayerNeurons=[32, 32, 32, 22, 22, 18], **one)))
    assert s.regressionModelInfo("big")["nInputs"] == 1


# ---- 5: parameter counts -----------------------------------------------------------------------------------------------------------------------
def test_parameter_counts(emu):
    want = {"nn3": 4 * 3 + 3 + 3 + 1, "nn534": 5 * 5 + 5 * 3 + 3 * 4 + 4 + 5 + 3 + 4 + 1, "nn2020": 541, "rbf1": 7, "rbf7": 7 * 11}
    for name, n in want.items():
        i, d = specs(RM.MODELS[name])
        assert RM.n_parameters(RM.MODELS[name]) == n == emu.emu_reg_n_parameters(i.ctypes.data_as(ip), dptr(d))


# ---- refusals and the Python layer, no device needed --------------------------------------------------------------------------------------------
def solver(case, **extra):
    opts = {"solverName": case.solver_name, "normalizeStates": {"U": 10.0, "p": 50.0, "nuTilda": 1e-3, "phi": 1.0}, "adjEqnOption": {"printInfo": 0}}
    opts.update(extra)
    return pyDASolvers((case.solver_name + " -python").encode(), opts, case=case)


def reg(**models):
    return dict(active=True, **models)


def test_inactive_option_defines_nothing():
    s = solver(channel_case(4, 3, 3), regressionModel=dict(active=False, m=dict(modelType="nonsense")))
    assert s._regressionModels == []
    with pytest.raises(_capi.DASError, match="no model m"):
        s.regressionModelInfo("m")


def test_info_and_input_size_are_keyed_by_the_model_name():
    case = channel_case(4, 3, 3)
    s = solver(case, regressionModel=reg(b_model=RM.MODELS["nn2020"], a_model=RM.MODELS["rbf7"]),
               inputInfo={"b_model": {"type": "regressionPar", "components": ["solver"]}, "other": {"type": "regressionPar"}})
    assert s._regressionModels == ["b_model", "a_model"]  # the order of the dictionary, not of the names
    info = s.regressionModelInfo("b_model")
    assert (info["nParameters"], info["nInputs"], info["modelType"]) == (541, 4, "neuralNetwork")
    assert s.regressionModelInfo("a_model")["nParameters"] == 77
    assert s.getInputSize("b_model", "regressionPar") == 541
    with pytest.raises(_capi.DASError, match="other"):
        s.getInputSize("other", "regressionPar")
    assert not hasattr(s, "getNRegressionParameters")
    p = RM.parameters(RM.MODELS["nn2020"])
    assert np.array_equal(s.getRegressionParameters("b_model"), np.zeros(541))  # zero until set, as in the reference
    s.setSolverInput("b_model", "regressionPar", 541, p)
    assert np.array_equal(s.getRegressionParameters("b_model"), p)
    with pytest.raises(_capi.DASError, match="540 values given, the model has 541"):
        s.setSolverInput("b_model", "regressionPar", 540, p[:540])


BAD = [
    (dict(modelType="externalTensorFlow"), "externalTensorFlow"),
    (dict(modelType="forest"), "modelType forest"),
    (dict(inputNames=["VoS", "KoU2", "chiSA", "PSoSS"]), "KoU2"),
    (dict(inputNames=["VoS", "ReWall", "chiSA", "PSoSS"]), "ReWall"),
    (dict(inputNames=["VoS", "TauoK", "chiSA", "PSoSS"]), "TauoK"),
    (dict(inputNames=["VoS", "CoP", "chiSA", "PSoSS"]), "CoP"),
    (dict(inputNames=["VoS", "PoD_dt", "chiSA", "PSoSS"]), "PoD_dt"),
    (dict(inputNames=["VoS", "Qcrit", "chiSA", "PSoSS"]), "inputName Qcrit not supported"),
    (dict(outputName="alphaPorosity"), "outputName alphaPorosity"),
    (dict(inputShift=[0.0, 0.0, 0.0]), "inputShift"),
    (dict(inputScale=[1.0] * 5), "inputScale"),
    (dict(activationFunction="gelu"), "activationFunction gelu"),
    # cap and cap + 1
    (dict(hiddenLayerNeurons=[33]), "DAS_REG_MAX_WIDTH"),
    (dict(hiddenLayerNeurons=[4] * 7), "DAS_REG_MAX_LAYERS"),
    (dict(modelType="radialBasisFunction", nRBFs=65), "DAS_REG_MAX_RBFS"),
    (dict(inputNames=["VoS"] * 9, inputShift=[0.0] * 9, inputScale=[1.0] * 9), "DAS_REG_MAX_INPUTS"),
    (dict(inputNames=["VoS"] * 8, inputShift=[0.0] * 8, inputScale=[1.0] * 8, hiddenLayerNeurons=[32] * 5), "DAS_REG_MAX_PARAMS"),
]


@pytest.mark.parametrize("change,word", BAD, ids=[w for _, w in BAD])
def test_refusals_name_the_offending_key(change, word):
    with pytest.raises(_capi.DASError, match=word) as e:
        solver(channel_case(4, 3, 3), regressionModel=reg(theModel=dict(RM.MODELS["nn3"], **change)))
    assert "theModel" in str(e.value)


def test_the_caps_themselves_are_admitted():
    eight = dict(inputNames=["VoS", "PoD", "chiSA", "pGradStream", "PSoSS", "SCurv", "UOrth", "VoS"], inputShift=[0.0] * 8, inputScale=[1.0] * 8)
    s = solver(channel_case(4, 3, 3), regressionModel=reg(
        wide=dict(RM.MODELS["nn3"], hiddenLayerNeurons=[32] * 4, **eight), deep=dict(RM.MODELS["nn3"], hiddenLayerNeurons=[8] * 6),
        rbf=dict(RM.MODELS["rbf7"], nRBFs=64, **eight)))
    assert s.regressionModelInfo("wide")["nParameters"] == 3489 and s.regressionModelInfo("rbf")["nParameters"] == 64 * 17
    with pytest.raises(_capi.DASError, match="DAS_REG_MAX_MODELS"):
        solver(channel_case(4, 3, 3), regressionModel=reg(**{f"m{k}": RM.MODELS["nn3"] for k in range(5)}))


@pytest.mark.parametrize("make", [lambda: rho_channel_case(4, 3, 3), lambda: heat_transfer_case(4, 3, 3, kappa=200.0)],
                         ids=["DARhoSimpleFoam", "DAHeatTransferFoam"])
def test_other_solvers_are_refused_by_name(make):
    case = make()
    with pytest.raises(_capi.DASError, match="regressionModel.*DASimpleFoam only.*" + case.solver_name):
        solver(case, regressionModel=reg(m=RM.MODELS["nn3"]))
    s = solver(case)
    sp = _capi.reg_spec(RM.MODELS["nn3"])
    assert _capi.lib().das_define_regression_model(s._h, b"m", C.byref(sp)) < 0
    assert "DASimpleFoam only" in _capi.lib().das_last_error().decode()


def test_field_input_and_volsum_objective_on_betaFINuTilda_are_refused_with_a_model():
    case = channel_case(4, 3, 3)
    with pytest.raises(_capi.DASError, match="beta_in.*betaFINuTilda"):
        solver(case, regressionModel=reg(m=RM.MODELS["nn3"]), inputInfo={"beta_in": {"type": "field", "fieldName": "betaFINuTilda", "fieldType": "scalar"}})
    with pytest.raises(_capi.DASError, match="betaSum"):
        solver(case, regressionModel=reg(m=RM.MODELS["nn3"]),
               function={"betaSum": {"type": "variableVolSum", "source": "allCells", "varName": "betaFINuTilda", "varType": "scalar", "index": 0, "isSquare": 0,
                                     "multiplyVol": 1, "divByTotalVol": 0, "scale": 1.0}})
    s = solver(case, regressionModel=reg(m=RM.MODELS["nn3"]))
    assert _capi.lib().das_set_field(s._h, b"betaFINuTilda", dptr(np.ones(case.mesh.n_cells))) < 0
    assert "regressionModel" in _capi.lib().das_last_error().decode()
    assert _capi.lib().das_simple_iteration(s._h, 1, 0.3, 1e-12, 100, None) < 0
    assert "regressionModel" in _capi.lib().das_last_error().decode()
    owned = np.ones(s.getNLocalAdjointStates(), dtype=np.uint8)
    assert _capi.lib().das_set_owned_mask(s._h, owned.ctypes.data_as(C.POINTER(C.c_ubyte))) < 0
    assert "sharded" in _capi.lib().das_last_error().decode()


def test_sharded_wrappers_refuse_the_option():
    from dafoam_amd.distributed import refuse_fv_source

    with pytest.raises(_capi.DASError, match="regressionModel.*sharded"):
        refuse_fv_source({"regressionModel": reg(m=RM.MODELS["nn3"])})
    refuse_fv_source({"regressionModel": {"active": False}})


def test_connectivity_gains_p_only_with_a_feature_that_reads_grad_p():
    """nuTildaRes lists p at levels 0 and 1 exactly when pGradStream or PSoSS is an input; otherwise the patterns are the ones without a model"""
    case = channel_case(5, 4, 3)
    N = case.mesh.n_cells

    def con(s, pc):
        s.runColoring()  # host graph work: no device needed
        A = s.getConnectivity(pc)
        A.sort_indices()
        return A.indptr, A.indices, A.shape[0]

    plain = solver(case)
    nop = solver(case, regressionModel=reg(m=RM.MODELS["nn3_nop"]))
    withp = solver(case, regressionModel=reg(m=RM.MODELS["nn3"]))
    for pc in (0, 1):
        rp0, ci0, n = con(plain, pc)
        rp1, ci1, _ = con(nop, pc)
        rp2, ci2, _ = con(withp, pc)
        assert np.array_equal(rp0, rp1) and np.array_equal(ci0, ci1)
        for c in range(N):
            row = 4 * N + c
            a, b = set(ci0[rp0[row]:rp0[row + 1]]), set(ci2[rp2[row]:rp2[row + 1]])
            extra = b - a
            assert a <= b and 3 * N + c in extra and all(3 * N <= j < 4 * N for j in extra) and len(extra) >= 2
        # every other row is untouched
        keep = np.ones(n, dtype=bool)
        keep[4 * N:5 * N] = False
        assert all(np.array_equal(ci0[rp0[r]:rp0[r + 1]], ci2[rp2[r]:rp2[r + 1]]) for r in np.flatnonzero(keep))
