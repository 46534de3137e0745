// TEST HARNESS ONLY (never linked into libdafoam_amd.so, never used by the product path).
// Runs the bodies that the HIP kernels k_heat_grad / k_heat wrap (body_heat_grad, body_heat, csrc/das_kernels.hpp) in plain host loops,
// with double and dual-number states and with dual-number metrics, so that the CPU-only test tier can check them against the numpy
// restatement (tests/test_heat_transfer_cpu.py).
#include "../../dafoam_amd/csrc/das_case.hpp"
#include "../../dafoam_amd/csrc/das_geom.hpp"

using namespace das;

template <class T, class MV>
static void heat_on(const MV& m, const ResParams& prm, const std::vector<T>& W, std::vector<T>& R) {
    std::vector<T> gT(3 * (size_t)m.nC);
    for (int c = 0; c < m.nC; c++) body_heat_grad<T>(c, m, prm, W.data(), gT.data());
    for (int c = 0; c < m.nC; c++) body_heat<T>(c, m, prm, W.data(), gT.data(), R.data());
}

static ResParams params_of(const CaseParams& cp, int isPC, int normalized) {
    Options opt;
    if (!normalized) opt.s["normalizeResiduals"] = "URes,pRes";
    return make_params(cp, opt, isPC);
}

// TRes at the states Win (n = the cells); dir: the forward tangent of the states -> Rd; normalized: TRes is listed in normalizeResiduals
extern "C" int emu_heat_residual(const das_case_t* c, const double* Win, long long n, int isPC, int normalized, const double* dir, double* Rv, double* Rd) {
    try {
        Mesh mesh;
        mesh.build(c);
        CaseParams cp;
        cp.from_case(c);
        if (cp.solver != DAS_SOLVER_HEATTRANSFERFOAM || n != mesh.nC) throw std::runtime_error("a DAHeatTransferFoam case and one state per cell expected");
        const ResParams prm = params_of(cp, isPC, normalized);
        if (!dir) {
            std::vector<double> W(Win, Win + n), R(n);
            heat_on<double>(host_view(mesh), prm, W, R);
            for (long long i = 0; i < n; i++) Rv[i] = R[i];
        } else {
            std::vector<Dual<1>> W(n), R(n);
            for (long long i = 0; i < n; i++) { W[i].v = Win[i]; W[i].d[0] = dir[i]; }
            heat_on<Dual<1>>(host_view(mesh), prm, W, R);
            for (long long i = 0; i < n; i++) { Rv[i] = R[i].v; Rd[i] = R[i].d[0]; }
        }
        return 0;
    } catch (const std::exception& e) {
        fprintf(stderr, "emu_heat_residual: %s\n", e.what());
        return -1;
    }
}

// dTRes/dX . dX with the metrics as dual numbers (points X + eps dX through the bodies of das_geom.hpp), states without tangents
extern "C" int emu_heat_geom(const das_case_t* c, const double* Win, long long n, const double* dX, double* Rd) {
    try {
        Mesh mesh;
        mesh.build(c);
        CaseParams cp;
        cp.from_case(c);
        if (cp.solver != DAS_SOLVER_HEATTRANSFERFOAM || n != mesh.nC) throw std::runtime_error("a DAHeatTransferFoam case and one state per cell expected");
        const ResParams prm = params_of(cp, 0, 1);
        typedef Dual<1> D;
        std::vector<D> P(3 * (size_t)mesh.nP);
        for (size_t i = 0; i < P.size(); i++) { P[i].v = mesh.points[i]; P[i].d[0] = dX[i]; }
        std::vector<FaceGeomT<D>> fg(mesh.nF);
        std::vector<CellGeomT<D>> cg(mesh.nC);
        const GeomTopo t = mesh.geom_topo();
        for (int f = 0; f < mesh.nF; f++) geom_face<D>(f, t, P.data(), fg[f]);
        for (int k = 0; k < mesh.nC; k++) { geom_cell<D>(k, t, fg.data(), cg[k]); cg[k].y = D(mesh.cg[k].y); }
        for (int f = 0; f < mesh.nF; f++) geom_weights<D>(f, t, cg.data(), fg.data(), fg[f]);
        DevMeshT<D> m;
        m.nC = mesh.nC; m.nF = mesh.nF; m.nIF = mesh.nIF;
        m.fg = fg.data(); m.cg = cg.data();
        m.cf_ptr = mesh.cf_ptr.data(); m.cf_face = mesh.cf_face.data(); m.cf_other = mesh.cf_other.data();
        m.owner = mesh.owner.data(); m.neigh = mesh.neighbour.data();
        m.bpatch = mesh.bface_patch.data(); m.bc = mesh.bc.data(); m.cyc = mesh.cyc_face.data();
        m.mixed = mesh.mixed.empty() ? nullptr : mesh.mixed.data();
        std::vector<D> W(n), R(n);
        for (long long i = 0; i < n; i++) W[i] = D(Win[i]);
        heat_on<D>(m, prm, W, R);
        for (long long i = 0; i < n; i++) Rd[i] = R[i].d[0];
        return 0;
    } catch (const std::exception& e) {
        fprintf(stderr, "emu_heat_geom: %s\n", e.what());
        return -1;
    }
}

// per boundary face faces[k]: out[k] = T of the owner cell, out[nf + k] = kappa(T_b) / d (body_thermal_coupling_solid), whf[k] = the
// wallHeatFlux summand kappa(T_b) snGrad(T) (body_facefn_solid), both under wallDistanceMethod default (custom = 0) or daCustom (1)
extern "C" int emu_heat_faces(const das_case_t* c, const double* Win, long long n, const int* faces, int nf, int custom, double* out, double* whf) {
    try {
        Mesh mesh;
        mesh.build(c);
        CaseParams cp;
        cp.from_case(c);
        if (cp.solver != DAS_SOLVER_HEATTRANSFERFOAM || n != mesh.nC) throw std::runtime_error("a DAHeatTransferFoam case and one state per cell expected");
        const ResParams prm = params_of(cp, 0, 1);
        const DevMesh m = host_view(mesh);
        const double dir[3] = {0.0, 0.0, 0.0};
        for (int k = 0; k < nf; k++) {
            if (faces[k] < mesh.nIF || faces[k] >= mesh.nF) throw std::runtime_error("not a boundary face");
            body_thermal_coupling_solid<double>(faces[k], m, prm, Win, custom != 0, out[k], out[nf + k]);
            whf[k] = body_facefn_solid<double>(faces[k], m, prm, Win, DAS_FN_WALLHEATFLUX | (custom ? DAS_FN_ALT_BIT : 0), dir);
        }
        return 0;
    } catch (const std::exception& e) {
        fprintf(stderr, "emu_heat_faces: %s\n", e.what());
        return -1;
    }
}

// kappa(T) of the Horner evaluation, value by value
extern "C" int emu_heat_kappa(const das_case_t* c, int n, const double* T, double* out) {
    try {
        CaseParams cp;
        cp.from_case(c);
        const ResParams prm = params_of(cp, 0, 1);
        for (int k = 0; k < n; k++) out[k] = kappa_of<double>(prm, T[k]);
        return 0;
    } catch (const std::exception& e) {
        fprintf(stderr, "emu_heat_kappa: %s\n", e.what());
        return -1;
    }
}
