"""The regression models of the reference restated in numpy, from the text of DARegression.C (calcInputFeatures :164-352, compute :354-650,
nParameters :652-710, checkOutput :712-773) and DASpalartAllmaras.C (getTurbProdOverDestruct :601-622 with chi, fv1, fv2, Stilda, fw of
:124-178): plain loops over cells and neurons, OpenFOAM's tensor algebra spelled out.  It shares no code with csrc/das_regression.hpp.

gradU[c, i, j] = d_i U_j (fvc::grad(U)), so
    U & gradU   -> sum_i U_i gradU[i, j]        gradU & U -> sum_j gradU[i, j] U_j
    symm(T) = (T + T^T) / 2, skew(T) = (T - T^T) / 2, mag(T) = sqrt(T && T) (all nine components), mag(v) = sqrt(v & v), mag(s) = |s|.
Every array keeps the dtype of its inputs (float64, or longdouble for the finite-difference checks)."""
import math

import numpy as np

FEATURES = ("VoS", "PoD", "chiSA", "pGradStream", "PSoSS", "SCurv", "UOrth")
SA = dict(sigmaNut=0.66666, kappa=0.41, Cb1=0.1355, Cb2=0.622, Cw2=0.3, Cw3=2.0, Cv1=7.1, Cs=0.3)
SA["Cw1"] = SA["Cb1"] / SA["kappa"] ** 2 + (1.0 + SA["Cb2"]) / SA["sigmaNut"]


def n_parameters(model, nInputs=None):
    """DARegression::nParameters"""
    nIn = len(model["inputNames"]) if nInputs is None else nInputs
    if model["modelType"] == "neuralNetwork":
        h = list(model["hiddenLayerNeurons"])
        n = nIn * h[0]
        for layer in range(1, len(h)):
            n += h[layer] * h[layer - 1]
        n += h[-1] * 1
        for layer in range(len(h)):
            n += h[layer]
        return n + 1
    if model["modelType"] == "radialBasisFunction":
        return model["nRBFs"] * (2 * nIn + 1)
    raise ValueError(model["modelType"])


def _mag_tensor(T):
    return np.sqrt((T * T).sum())


def _mag_vector(v):
    return np.sqrt((v * v).sum())


def prod_over_destruct(nuTilda, nu, gradU, y):
    """getTurbProdOverDestruct of one cell (incompressible: rho = phase = 1)"""
    chi = nuTilda / nu
    chi3 = chi * chi * chi
    fv1 = chi3 / (chi3 + SA["Cv1"] ** 3)
    fv2 = 1.0 - chi / (1.0 + chi * fv1)
    Omega = math.sqrt(2.0) * _mag_tensor(0.5 * (gradU - gradU.T))
    k2y2 = (SA["kappa"] * y) ** 2
    Stilda = max(Omega + fv2 * nuTilda / k2y2, SA["Cs"] * Omega)
    r = min(nuTilda / (max(Stilda, 1e-15) * k2y2), 10.0)
    g = r + SA["Cw2"] * (r**6 - r)
    fw = g * ((1.0 + SA["Cw3"] ** 6) / (g**6 + SA["Cw3"] ** 6)) ** (1.0 / 6.0)
    P = SA["Cb1"] * Stilda * nuTilda
    D = SA["Cw1"] * fw * (nuTilda / y) ** 2
    return P / (D + P + 1e-16)


def feature(name, U, nuTilda, nu, gradU, gradP, y):
    """one feature of one cell before shift and scale"""
    if name == "VoS":
        magOmega = _mag_tensor(0.5 * (gradU - gradU.T))
        magS = _mag_tensor(0.5 * (gradU + gradU.T))
        return magOmega / (magS + magOmega + 1e-16)
    if name == "PoD":
        return prod_over_destruct(nuTilda, nu, gradU, y)
    if name == "chiSA":
        return nuTilda / (nu + nuTilda + 1e-16)
    if name == "pGradStream":
        UdP = (U * gradP).sum()
        return UdP / (_mag_vector(U) * _mag_vector(gradP) + abs(UdP) + 1e-16)
    if name == "PSoSS":
        diagUGrad = np.array([gradU[0, 0], gradU[1, 1], gradU[2, 2]])
        return _mag_vector(gradP) / (_mag_vector(gradP) + abs(3.0 * (U * diagUGrad).sum()) + 1e-16)
    UgU = np.array([sum(U[i] * gradU[i, j] for i in range(3)) for j in range(3)])  # U & gradU
    if name == "SCurv":
        return _mag_vector(UgU) / (abs((U * U).sum()) + _mag_vector(UgU) + 1e-16)
    if name == "UOrth":
        gUU = np.array([sum(gradU[i, j] * U[j] for j in range(3)) for i in range(3)])  # gradU & U
        UgUU = abs((UgU * U).sum())
        return UgUU / (_mag_vector(U) * _mag_vector(gUU) + UgUU + 1e-16)
    raise ValueError(f"inputName: {name} not supported")


def features(model, U, nuTilda, nu, gradU, gradP, y):
    """(nCells, nInputs): (f + inputShift) * inputScale"""
    N = U.shape[0]
    out = np.zeros((N, len(model["inputNames"])), dtype=U.dtype)
    for c in range(N):
        for k, name in enumerate(model["inputNames"]):
            out[c, k] = (feature(name, U[c], nuTilda[c], nu, gradU[c], gradP[c], y[c]) + model["inputShift"][k]) * model["inputScale"][k]
    return out


def raw_output(model, par, feat):
    """outputScale * (out + outputShift) per cell, before checkOutput; feat (nCells, nInputs)"""
    N, nIn = feat.shape
    dt = np.result_type(feat.dtype, np.asarray(par).dtype)
    out = np.zeros(N, dtype=dt)
    one = dt.type(1)
    for c in range(N):
        if model["modelType"] == "neuralNetwork":
            k = 0
            prev = [feat[c, j] for j in range(nIn)]
            for nNeurons in model["hiddenLayerNeurons"]:
                cur = []
                for _ in range(nNeurons):
                    v = dt.type(0)
                    for x in prev:
                        v += x * par[k]
                        k += 1
                    v += par[k]
                    k += 1
                    act = model["activationFunction"]
                    if act == "sigmoid":
                        v = one / (one + np.exp(-v))
                    elif act == "tanh":
                        v = (one - np.exp(-2 * v)) / (one + np.exp(-2 * v))
                    elif act == "relu":
                        if v < 0:
                            v = model.get("leakyCoeff", 0.0) * v
                    else:
                        raise ValueError("activationFunction not valid")
                    cur.append(v)
                prev = cur
            o = dt.type(0)
            for x in prev:
                o += x * par[k]
                k += 1
            o += par[k]
        else:
            dP = 2 * nIn + 1
            o = dt.type(0)
            for i in range(model["nRBFs"]):
                e = dt.type(0)
                for j in range(nIn):
                    A = (feat[c, j] - par[dP * i + 2 * j]) * (feat[c, j] - par[dP * i + 2 * j])
                    B = 2 * par[dP * i + 2 * j + 1] * par[dP * i + 2 * j + 1]
                    e += A / B
                o += par[dP * i + dP - 1] * np.exp(-e)
        out[c] = model["outputScale"] * (o + model["outputShift"])
    return out


def check_output(model, out):
    """checkOutput: (the bounded field, a mask per cell with bit 0 NaN, bit 1 Inf, bit 2 bounded)"""
    out = out.copy()
    mask = np.zeros(out.size, dtype=np.int64)
    for c in range(out.size):
        if np.isnan(out[c]):
            out[c] = model["defaultOutputValue"]
            mask[c] |= 1
        if np.isinf(out[c]):
            out[c] = model["defaultOutputValue"]
            mask[c] |= 2
        if out[c] > model["outputUpperBound"]:
            out[c] = model["outputUpperBound"]
            mask[c] |= 4
        if out[c] < model["outputLowerBound"]:
            out[c] = model["outputLowerBound"]
            mask[c] |= 4
    return out, mask


def fail_counts(mask):
    return [int(((mask >> q) & 1).sum()) for q in range(3)]


def beta(model, par, feat):
    return check_output(model, raw_output(model, par, feat))


def dbeta_dpar_fd(model, par, feat, g, rel=1e-6, only=None):
    """sum_c g[c] d beta_c / d par_k by central differences in longdouble, the bounds included (a clipped cell contributes nothing);
    only = k: that entry alone, as a float"""
    L = np.longdouble
    p0 = np.asarray(par, dtype=L)
    f = np.asarray(feat, dtype=L)
    gl = np.asarray(g, dtype=L)
    out = np.zeros(p0.size)
    for k in (range(p0.size) if only is None else [only]):
        h = L(rel) * max(abs(p0[k]), L(1e-2))
        pp, pm = p0.copy(), p0.copy()
        pp[k] += h
        pm[k] -= h
        bp, _ = beta(model, pp, f)
        bm, _ = beta(model, pm, f)
        out[k] = float((gl * (bp - bm)).sum() / (2 * h))
    return out if only is None else float(out[only])


# ---- the models and the flow side shared by tests/test_regression_model_cpu.py and tests/test_gpu_regression_model.py ------------------
def _model(**kw):
    m = dict(outputName="betaFINuTilda", outputShift=1.0, outputScale=1.0, outputUpperBound=1e1, outputLowerBound=-1e1, defaultOutputValue=1.0)
    m.update(kw)
    n = len(m["inputNames"])
    m.setdefault("inputShift", [0.05 * (k - 1) for k in range(n)])
    m.setdefault("inputScale", [1.0 + 0.1 * k for k in range(n)])
    return m


MODELS = {
    # [3] sigmoid; PSoSS reads grad(p)
    "nn3": _model(modelType="neuralNetwork", inputNames=["VoS", "PoD", "chiSA", "PSoSS"], hiddenLayerNeurons=[3], activationFunction="sigmoid"),
    # the reference's own example shape, all seven features but PoD and PSoSS
    "nn534": _model(modelType="neuralNetwork", inputNames=["VoS", "chiSA", "pGradStream", "SCurv", "UOrth"], hiddenLayerNeurons=[5, 3, 4],
                    activationFunction="tanh"),
    # 541 parameters: more than one workgroup of the backward kernel has threads
    "nn2020": _model(modelType="neuralNetwork", inputNames=["VoS", "PoD", "chiSA", "pGradStream"], hiddenLayerNeurons=[20, 20], activationFunction="relu",
                     leakyCoeff=0.1),
    # no feature reads grad(p): the connectivity stays as it is
    "nn3_nop": _model(modelType="neuralNetwork", inputNames=["VoS", "PoD", "chiSA", "SCurv"], hiddenLayerNeurons=[3], activationFunction="sigmoid"),
    "rbf1": _model(modelType="radialBasisFunction", inputNames=["VoS", "chiSA", "UOrth"], nRBFs=1),
    "rbf7": _model(modelType="radialBasisFunction", inputNames=["VoS", "PoD", "chiSA", "PSoSS", "SCurv"], nRBFs=7),
}


def parameters(model, seed=0, amp=0.6):
    """a parameter vector with every entry live: network weights in (-amp, amp); RBF means inside the feature range, standard deviations in
    (0.6, 1.4), weights in (-amp, amp)"""
    rng = np.random.default_rng(1234 + seed)
    n = n_parameters(model)
    p = amp * (2.0 * rng.random(n) - 1.0)
    if model["modelType"] == "radialBasisFunction":
        dP = 2 * len(model["inputNames"]) + 1
        for i in range(model["nRBFs"]):
            for j in range(len(model["inputNames"])):
                p[dP * i + 2 * j] = 0.5 * rng.random()
                p[dP * i + 2 * j + 1] = 0.6 + 0.8 * rng.random()
    return p


def clipped(model, lo=0.9, hi=1.1):
    """the model with bounds that the outputs of parameters() cross on some cells and not on others (the tests check that on the restatement)"""
    return dict(model, outputLowerBound=lo, outputUpperBound=hi)


def flow_inputs(case, g, W):
    """(U, nuTilda, gradU, gradP, y) of the states W: the gradients are the oracle's Gauss gradients (oracle.residual.simple_residual)"""
    from oracle.residual import simple_residual, unpack_simple

    _, parts = simple_residual(case, g, W, return_parts=True)
    U, _, nuT, _ = unpack_simple(W, g.nC, g.nF)
    return U, nuT, parts["gradU"], parts["gradP"], np.asarray(case.y_wall)


def restated_beta(case, g, W, models):
    """betaFINuTilda of the states W: models = [(model, parameters), ...] in the order of the option; the last one wins.  Returns
    (beta, mask of the last model)"""
    U, nuT, gradU, gradP, y = flow_inputs(case, g, W)
    b = m = None
    for model, par in models:
        b, m = beta(model, par, features(model, U, nuT, case.nu, gradU, gradP, y))
    return b, m


def restated_residual(case, g, W, models, **kw):
    """R(W) with the models active: the oracle's residual with betaFINuTilda of the restatement at the same states"""
    import copy

    from oracle.residual import simple_residual

    c = copy.copy(case)
    c.beta_fi = restated_beta(case, g, W, models)[0]
    return simple_residual(c, g, W, **kw)


def stirred_states(case, seed=7, rel=0.05):
    """the states of the case with every cell value moved by up to rel of its field's scale: no gradient is zero anywhere"""
    rng = np.random.default_rng(seed)
    W = np.array(case.states, dtype=np.float64)
    N = case.mesh.n_cells
    hasT = bool(getattr(case, "has_T", False))
    blocks = [(0, 3 * N, 10.0), (3 * N, 4 * N, 50.0)] + ([(4 * N, 5 * N, 300.0), (5 * N, 6 * N, 1e-3)] if hasT else [(4 * N, 5 * N, 1e-3)])
    for a, b, s in blocks:
        W[a:b] += rel * s * (2.0 * rng.random(b - a) - 1.0)
    nt = slice(5 * N, 6 * N) if hasT else slice(4 * N, 5 * N)
    W[nt] = np.abs(W[nt]) + 1e-5
    return W


class CpuPrimal:
    """The primal of restatement + oracle on the CPU: R(W, theta) = 0 with betaFINuTilda = model(W, theta), by quasi-Newton steps with the
    oracle's complex-step Jacobian at frozen beta (the model's share of the Jacobian is small: the steps contract by orders each).  The
    first solve starts from the oracle's converged SIMPLE primal and refreshes the Jacobian; every later solve starts from the first
    solution, reuses its factorisation and takes a fixed number of steps, so that each one ends on the round-off floor of the residual
    whatever the size of the parameter step."""

    def __init__(self, case, g, model, par, norm_states):
        import scipy.sparse.linalg as spla

        from oracle import jacobian as J
        from oracle.primal import solve_primal
        from oracle.residual import residual

        self.case, self.g, self.model, self.residual, self.spla, self.J = case, g, model, residual, spla, J
        self.sc = J.state_scales(case, g, norm_states)
        self.con = J.connectivity(case, g)
        self.col, _ = J.greedy_coloring(self.con)
        self.ref = np.linalg.norm(residual(case, g, case.states))
        W, _ = solve_primal(case, g, max_iters=800, tol=1e-11)
        self.lu = None
        for it in range(40):
            R, cb = self._residual(W, par)
            if np.linalg.norm(R) <= 1e-13 * self.ref:
                break
            if it % 4 == 0:
                self.lu = spla.splu(J.jacobian_colored(cb, g, W, self.con, self.col, self.sc, mode="cs", lower_bound=0).T.tocsc())
            W = W + self.sc * self.lu.solve(-R)
        else:
            raise AssertionError("the CPU primal did not converge")
        self.W0 = W

    def _residual(self, W, par):
        import copy

        cb = copy.copy(self.case)
        cb.beta_fi = restated_beta(self.case, self.g, W, [(self.model, par)])[0]
        return self.residual(cb, self.g, W), cb

    def solve(self, par, steps=12):
        W = self.W0.copy()
        for _ in range(steps):
            W = W + self.sc * self.lu.solve(-self._residual(W, par)[0])
        return W
