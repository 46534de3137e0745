// TEST HARNESS ONLY (never linked into libdafoam_amd.so, never used by the product path).
// Runs body_heat_source (csrc/das_kernels.hpp) - the body the kernels k_hs_partial / k_hs_apply of csrc/das_heatsource.hpp wrap - in plain host
// loops with double scalars, with dual-number parameters and with dual-number metrics, and body_heat with the src pointer set, so that the
// CPU-only test tier can check them against the numpy restatement (tests/test_heat_source_cpu.py).
#include "../../dafoam_amd/csrc/das_case.hpp"
#include "../../dafoam_amd/csrc/das_geom.hpp"

using namespace das;

// s_c of a cylinderSmooth source with the parameters pars9 and eps at every cell -> sv; snapCell >= 0: the centre is C of that cell.
// dpar (9 tangents of the parameters) or dX (3 nP tangents of the points), not both: the forward tangent of s -> sd
extern "C" int emu_hs_shape(const das_case_t* c, const double* pars9, double eps, int snapCell, const double* dpar, const double* dX, double* sv, double* sd) {
    try {
        Mesh mesh;
        mesh.build(c);
        typedef Dual<1> D;
        if (dpar && dX) throw std::runtime_error("one kind of tangent at a time");
        if (snapCell >= mesh.nC) throw std::runtime_error("no such cell");
        if (dX) {
            std::vector<D> P(3 * (size_t)mesh.nP);
            for (size_t i = 0; i < P.size(); i++) { P[i].v = mesh.points[i]; P[i].d[0] = dX[i]; }
            std::vector<FaceGeomT<D>> fg(mesh.nF);
            std::vector<CellGeomT<D>> cg(mesh.nC);
            const GeomTopo t = mesh.geom_topo();
            for (int f = 0; f < mesh.nF; f++) geom_face<D>(f, t, P.data(), fg[f]);
            for (int k = 0; k < mesh.nC; k++) geom_cell<D>(k, t, fg.data(), cg[k]);
            for (int k = 0; k < mesh.nC; k++) {
                D ctr[3] = {D(pars9[0]), D(pars9[1]), D(pars9[2])}, axis[3] = {D(pars9[3]), D(pars9[4]), D(pars9[5])};
                if (snapCell >= 0) for (int i = 0; i < 3; i++) ctr[i] = cg[snapCell].C[i];
                const D s = body_heat_source<D, D, D>(ctr, axis, D(pars9[6]), D(pars9[7]), eps, cg[k].C);
                sv[k] = s.v;
                sd[k] = s.d[0];
            }
        } else if (dpar) {
            D p[9];
            for (int i = 0; i < 9; i++) { p[i].v = pars9[i]; p[i].d[0] = dpar[i]; }
            if (snapCell >= 0) for (int i = 0; i < 3; i++) p[i] = D(mesh.cg[snapCell].C[i]);
            for (int k = 0; k < mesh.nC; k++) {
                const D s = body_heat_source<D, D, double>(p, p + 3, p[6], p[7], eps, mesh.cg[k].C);
                sv[k] = s.v;
                sd[k] = s.d[0];
            }
        } else {
            double p[9];
            for (int i = 0; i < 9; i++) p[i] = pars9[i];
            if (snapCell >= 0) for (int i = 0; i < 3; i++) p[i] = mesh.cg[snapCell].C[i];
            for (int k = 0; k < mesh.nC; k++) sv[k] = body_heat_source<double, double, double>(p, p + 3, p[6], p[7], eps, mesh.cg[k].C);
        }
        return 0;
    } catch (const std::exception& e) {
        fprintf(stderr, "emu_hs_shape: %s\n", e.what());
        return -1;
    }
}

// TRes at the states Win with the source field src (one value per cell; null: DevMeshT::src stays null)
extern "C" int emu_hs_residual(const das_case_t* c, const double* Win, long long n, int normalized, const double* src, double* Rv) {
    try {
        Mesh mesh;
        mesh.build(c);
        CaseParams cp;
        cp.from_case(c);
        if (cp.solver != DAS_SOLVER_HEATTRANSFERFOAM || n != mesh.nC) throw std::runtime_error("a DAHeatTransferFoam case and one state per cell expected");
        Options opt;
        if (!normalized) opt.s["normalizeResiduals"] = "URes,pRes";
        const ResParams prm = make_params(cp, opt, 0);
        DevMesh m = host_view(mesh);
        m.src = src;
        std::vector<double> gT(3 * (size_t)mesh.nC);
        for (int k = 0; k < mesh.nC; k++) body_heat_grad<double>(k, m, prm, Win, gT.data());
        for (int k = 0; k < mesh.nC; k++) body_heat<double>(k, m, prm, Win, gT.data(), Rv);
        return 0;
    } catch (const std::exception& e) {
        fprintf(stderr, "emu_hs_residual: %s\n", e.what());
        return -1;
    }
}
