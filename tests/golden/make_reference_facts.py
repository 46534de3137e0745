"""Generates tests/golden/reference_facts.json: the machine-checkable facts of the reference's sources that
tests/test_reference_pins.py pins the oracle and the product against (stencil tables, DAOPTION defaults, model
constants, Krylov configuration, dump-file conventions, the method lists of the Python / Cython front ends).

The fixture holds extracted DATA only (names, numbers, tables and whether a documented construct was found); the
tests read it instead of the reference checkout, so the suite runs from the repository alone.  Regenerate it when the
pinned reference changes:
    python tests/golden/make_reference_facts.py <path to the DAFoam checkout>"""
import ast
import json
import os
import re
import sys

here = os.path.dirname(os.path.abspath(__file__))
SOLVERS = ["DASimpleFoam", "DARhoSimpleFoam", "DATurboFoam", "DAScalarTransportFoam"]


def strip_comments(src):
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return re.sub(r"//[^\n]*", "", src)


def parse_level_tables(src, setter):
    """All `<setter>.set("NAME", { {..}, {..}, ... });` blocks of a reference source -> [(NAME, [[states lv0], [lv1], ...])].
    Identifiers (pName) are kept as bare words."""
    src = strip_comments(src)
    out = []
    for m in re.finditer(re.escape(setter) + r"\.set\(\s*\"(\w+)\"\s*,\s*\{(.*?)\}\s*\)\s*;", src, flags=re.S):
        levels = [[t.strip().strip('"') for t in grp.split(",") if t.strip()] for grp in re.findall(r"\{([^{}]*)\}", m.group(2))]
        out.append((m.group(1), levels))
    return out


class Reference:
    def __init__(self, root):
        self.root = root
        self.found = {}

    def text(self, rel):
        with open(os.path.join(self.root, rel)) as f:
            return f.read()

    def check(self, name, ok):
        self.found[name] = bool(ok)

    def stencil(self, solver, has_T=False):
        """{residual: levels} of a solver as the reference builds it: DAStateInfo<solver>.C + the SA model table, with the
        model state `nut` renamed to `nuTilda` (DASpalartAllmaras::correctModelStates / correctStateResidualModelCon)."""
        sa = self.text("src/adjoint/DAModel/DATurbulenceModel/DASpalartAllmaras.C")
        assert re.search(r'stateName == "nut"\)\s*\{\s*modelStates\[idxI\] = "nuTilda";', sa)  # the rename this function applies
        tabs = parse_level_tables(self.text(f"src/adjoint/DAStateInfo/DAStateInfo{solver[2:]}.C"), "stateResConInfo_")
        res = {}
        for name, lv in tabs:
            if name == "TRes" and solver == "DASimpleFoam" and not has_T:
                continue
            res[name] = [["nuTilda" if s == "nut" else s for s in level] for level in lv]
        if solver != "DAScalarTransportFoam":
            sa_tabs = parse_level_tables(sa, "allCon")
            assert [n for n, _ in sa_tabs] == ["nuTildaRes", "nuTildaRes"]  # incompressible first, compressible second (:364-383)
            assert re.search(r'turbModelType_ == "incompressible"\)\s*\{\s*allCon\.set', strip_comments(sa))
            lv = sa_tabs[0 if solver == "DASimpleFoam" else 1][1]
            res["nuTildaRes"] = [["p" if s == "pName" else s for s in level] for level in lv]
        return res

    def daoption(self):
        tree = ast.parse(self.text("dafoam/pyDAFoam.py"))
        cls = [n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == "DAOPTION"][0]
        init = [f for f in cls.body if isinstance(f, ast.FunctionDef) and f.name == "__init__"][0]
        return {st.targets[0].attr: ast.literal_eval(st.value) for st in init.body
                if isinstance(st, ast.Assign) and isinstance(st.targets[0], ast.Attribute)}

    def state_registration(self):
        """DAIndex.C registers adjStateNames by category; the order of the categories there is the state ordering."""
        idx = strip_comments(self.text("src/adjoint/DAIndex/DAIndex.C"))
        cats = ["volVectorStates", "volScalarStates", "modelStates", "surfaceScalarStates"]
        pos = {c: re.search(r'stateInfo_\["%s"\]' % c, idx).start() for c in cats}
        return sorted(cats, key=pos.get)

    def state_appends(self, solver):
        """{category: [state names in the order they are appended]} of DAStateInfo<solver>.C."""
        src = strip_comments(self.text(f"src/adjoint/DAStateInfo/DAStateInfo{solver[2:]}.C"))
        out = {}
        for cat, name in re.findall(r'\["(\w+States)"\]\.append\("(\w+)"\)', src):
            out.setdefault(cat, []).append(name)
        return out

    def spalart_allmaras(self):
        sa = strip_comments(self.text("src/adjoint/DAModel/DATurbulenceModel/DASpalartAllmaras.C"))
        coeffs = {m.group(1): float(m.group(2))
                  for m in re.finditer(r'lookupOrAddToDict\(\s*"(\w+)"\s*,\s*this->coeffDict_\s*,\s*([0-9.eE+-]+)\)', sa)}
        self.check("sa_cw1_from_cb1_kappa_cb2_sigma", re.search(r"Cw1_\(Cb1_ / sqr\(kappa_\) \+ \(1\.0 \+ Cb2_\) / sigmaNut_\)", sa))
        # functions of the model as the reference writes them (DASpalartAllmaras.C:124-172): fv1, fv2, the r clip at 10, Cs clip
        self.check("sa_fv1_chi3_over_chi3_plus_cv1_cubed", re.search(r"chi3 / \(chi3 \+ pow3\(Cv1_\)\)", sa))
        self.check("sa_fv2_one_minus_chi_over_one_plus_chi_fv1", re.search(r"1\.0 - chi / \(1\.0 \+ chi \* fv1\)", sa))
        self.check("sa_r_clipped_at_10", re.search(r"scalar\(10\.0\)", sa))
        self.check("sa_stilda_clip_cs_omega", re.search(r"Cs_ \* Omega", sa))
        return coeffs

    def spalding(self):
        wf = strip_comments(self.text("src/adjoint/DAMisc/nutUSpaldingWallFunctionDF/nutUSpaldingWallFunctionFvPatchScalarFieldDF.C"))
        clip = re.search(r"min\(kappa_ \* magUp\[facei\] / ut, ([0-9.]+)\)", wf)
        self.check("spalding_tolerance_guard_1e-14", re.search(r"tolerance_ != 1\.e-14", wf))
        max_iter = re.findall(r'maxIter_\((\d+)\)|lookupOrDefault<label>\("maxIter", (\d+)\)', wf)
        tol = re.findall(r'tolerance_\(([0-9.eE+-]+)\)|lookupOrDefault<scalar>\("tolerance", ([0-9.eE+-]+)\)', wf)
        self.check("spalding_nut_w_is_ut2_over_dudn_minus_nuw", re.search(r"sqr\(calcUTau\(magGradU\)\) / \(magGradU \+ ROOTVSMALL\) - nuw", wf))
        return {"exponent_clip": float(clip.group(1)) if clip else None,
                # the constructor default and the dictionary default of each setting
                "maxIter": [int(a or b) for a, b in max_iter],
                "tolerance": [float(a or b) for a, b in tol]}

    def incompressible_pmin(self):
        m = re.search(r'self\.defaultOptions\["primalVarBounds"\]\[1\]\["pMin"\] = (-?[0-9.eE+]+)', self.text("dafoam/pyDAFoam.py"))
        return float(m.group(1)) if m else None

    def krylov(self):
        le = strip_comments(self.text("src/adjoint/DALinearEqn/DALinearEqn.C"))
        ksp_type = re.search(r"KSPType kspObjectType = (\w+);", le)
        self.check("ksp_type_set_from_kspObjectType", re.search(r"KSPSetType\(ksp, kspObjectType\)", le))
        side = re.search(r"KSPSetPCSide\(ksp, (\w+)\)", le)
        names = ["KSP_GMRES_CGS_REFINE_IFNEEDED", "KSPGMRESModifiedGramSchmidtOrthogonalization", "useMGSO", "KSP_NORM_UNPRECONDITIONED",
                 "PCASM", "PCASMSetOverlap", "PCILU", "PCFactorSetLevels", "MAT_SHIFT_NONZERO", "KSPRICHARDSON"]
        # failure rule (DALinearEqn.C:422-434): fail only when BOTH ratios exceed gmresTolDiff
        self.check("failure_when_both_ratios_exceed_tol_diff",
                   re.search(r"if \(relResRatio > resDiff && absResRatio > resDiff\)\s*\{[^}]*return 1;", le, flags=re.S))
        self.check("rel_ratio_is_final_over_init_over_gmresRelTol",
                   re.search(r'relResRatio = finalResNorm / initResNorm / daOption_\.getSubDictOption<scalar>\("adjEqnOption", "gmresRelTol"\)', le))
        return {"ksp_type": ksp_type.group(1) if ksp_type else None, "pc_side": side.group(1) if side else None,
                "identifiers_used": sorted(n for n in names if n in le)}

    def partderiv(self):
        pd = strip_comments(self.text("src/adjoint/DAPartDeriv/DAPartDeriv.C"))
        ins = re.search(r"MatSetValue\(jacMat, (\w+), (\w+), val, INSERT_VALUES\)", pd)  # DAPartDeriv.C:194-197
        self.check("partderiv_uses_jacLowerBound", re.search(r"jacLowerBound", pd))
        # the phi columns are scaled by the face area in the perturbation (DAPartDeriv.C:283-311)
        self.check("partderiv_scales_by_magSf", re.search(r"magSf", pd))
        return {"matsetvalue_row_col": [ins.group(1), ins.group(2)] if ins else None}

    def dumps(self):
        ut = strip_comments(self.text("src/adjoint/DAUtility/DAUtility.C"))
        jc = strip_comments(self.text("src/adjoint/DAJacCon/DAJacCon.C"))
        sol = strip_comments(self.text("src/adjoint/DASolver/DASolver.C"))
        io_fns = ["writeMatrixBinary", "readMatrixBinary", "writeVectorBinary", "readVectorBinary"]
        viewer = ["PetscViewerBinaryOpen", "MatView", "VecView", "FILE_MODE_WRITE"]
        self.check("write_jacobians_dRdWT_or_all", re.search(r'writeJacobians\.found\("dRdWT"\) \|\| writeJacobians\.found\("all"\)', sol))
        return {"dautility_io_functions": [fn for fn in io_fns if re.search(r"void DAUtility::" + fn, ut)],
                "prefix_dot_bin_file_names": len(re.findall(r'fileNameStream << prefix << "\.bin";', ut)),
                "viewer_calls": [v for v in viewer if v in ut],
                # exists / calc / read: dRdWColoring_<nProcs>.bin
                "coloring_file_name_sites": len(re.findall(r'word fileName = modelType_ \+ "Coloring" \+ postFix \+ "_" \+ Foam::name\(nProcs\);', jc)),
                "jacobian_mat_names": sorted(set(re.findall(r'matName = "(\w+)";', sol)))}

    def pydasolvers_methods(self):
        src = self.text("src/pyDASolvers/pyDASolvers.pyx")
        cls = src[src.index("cdef class pyDASolvers"):]
        return sorted(set(n for n in re.findall(r"^\s+def\s+(\w+)\s*\(", cls, flags=re.M) if not n.startswith("__")))

    def pydafoam_methods(self):
        tree = ast.parse(self.text("dafoam/pyDAFoam.py"))
        return [f.name for c in tree.body if isinstance(c, ast.ClassDef) and c.name == "PYDAFOAM" for f in c.body if isinstance(f, ast.FunctionDef)]


def main(root):
    R = Reference(root)
    facts = {
        "stencil": {s: R.stencil(s) for s in SOLVERS},
        "stencil_simplefoam_with_T": R.stencil("DASimpleFoam", has_T=True),
        "daoption": R.daoption(),
        "state_registration_order": R.state_registration(),
        "state_appends": {s: R.state_appends(s) for s in ("DASimpleFoam", "DARhoSimpleFoam")},
        "spalart_allmaras_coeffs": R.spalart_allmaras(),
        "spalding": R.spalding(),
        "incompressible_pMin": R.incompressible_pmin(),
        "krylov": R.krylov(),
        "partderiv": R.partderiv(),
        "dumps": R.dumps(),
        "pydasolvers_methods": R.pydasolvers_methods(),
        "pydafoam_methods": R.pydafoam_methods(),
    }
    facts["found"] = R.found
    out = os.path.join(here, "reference_facts.json")
    with open(out, "w") as f:
        json.dump(facts, f, indent=1, sort_keys=True)
        f.write("\n")
    print("written", out)


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])
