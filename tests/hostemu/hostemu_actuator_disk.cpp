// TEST HARNESS ONLY (never linked into libdafoam_amd.so, never used by the product path).
// Runs body_actuator_disk (csrc/das_kernels.hpp) - the body the kernels k_ad_partial / k_ad_apply of csrc/das_actuatordisk.hpp wrap - in plain
// host loops with double scalars, with dual-number parameters and with dual-number metrics, and the DASimpleFoam residual bodies with the
// src3 pointer set (body_cell, or body_fcoef + body_bcoef + body_cell2), so that the CPU-only test tier can check them against the numpy
// restatement (tests/test_actuator_disk_cpu.py).
#include "../../dafoam_amd/csrc/das_case.hpp"
#include "../../dafoam_amd/csrc/das_geom.hpp"

using namespace das;

// f[0..4] = {f_x, f_y, f_z, fAxial, fCirc} of one disk at every cell -> fv (5 per cell); the scale is pars13[8].
// dpar (13 tangents of the parameters) or dX (3 nP tangents of the points), not both: the forward tangent -> fd.
// degenerate: the number of cells where the reference would divide by zero.
extern "C" int emu_ad_force(const das_case_t* c, int smooth, const double* pars13, double eps, double rotSign, const double* dpar, const double* dX, double* fv,
                            double* fd, int* degenerate) {
    try {
        Mesh mesh;
        mesh.build(c);
        typedef Dual<1> D;
        if (dpar && dX) throw std::runtime_error("one kind of tangent at a time");
        int deg = 0;
        if (dX) {
            std::vector<D> P(3 * (size_t)mesh.nP);
            for (size_t i = 0; i < P.size(); i++) { P[i].v = mesh.points[i]; P[i].d[0] = dX[i]; }
            std::vector<FaceGeomT<D>> fg(mesh.nF);
            std::vector<CellGeomT<D>> cg(mesh.nC);
            const GeomTopo t = mesh.geom_topo();
            for (int f = 0; f < mesh.nF; f++) geom_face<D>(f, t, P.data(), fg[f]);
            for (int k = 0; k < mesh.nC; k++) geom_cell<D>(k, t, fg.data(), cg[k]);
            const double* p = pars13;
            for (int k = 0; k < mesh.nC; k++) {
                D f[5];
                deg += body_actuator_disk<D, double, D>(smooth, p, p + 3, p[6], p[7], D(p[8]), p[9], p[10], p[11], eps, rotSign, cg[k].C, f);
                for (int i = 0; i < 5; i++) { fv[5 * k + i] = f[i].v; fd[5 * k + i] = f[i].d[0]; }
            }
        } else if (dpar) {
            D p[13];
            for (int i = 0; i < 13; i++) { p[i].v = pars13[i]; p[i].d[0] = dpar[i]; }
            for (int k = 0; k < mesh.nC; k++) {
                D f[5];
                deg += body_actuator_disk<D, D, double>(smooth, p, p + 3, p[6], p[7], p[8], p[9], p[10], p[11], eps, rotSign, mesh.cg[k].C, f);
                for (int i = 0; i < 5; i++) { fv[5 * k + i] = f[i].v; fd[5 * k + i] = f[i].d[0]; }
            }
        } else {
            const double* p = pars13;
            for (int k = 0; k < mesh.nC; k++)
                deg += body_actuator_disk<double, double, double>(smooth, p, p + 3, p[6], p[7], p[8], p[9], p[10], p[11], eps, rotSign, mesh.cg[k].C, fv + 5 * k);
        }
        if (degenerate) *degenerate = deg;
        return 0;
    } catch (const std::exception& e) {
        fprintf(stderr, "emu_ad_force: %s\n", e.what());
        return -1;
    }
}

// R(W) of DASimpleFoam with the source field src3 (3 per cell; null: DevMeshT::src3 stays null).  split: the cell pass through
// body_fcoef + body_bcoef + body_cell2 instead of body_cell.  normalized 0: no residual is normalised.
extern "C" int emu_ad_residual(const das_case_t* c, const double* Win, long long n, int split, int normalized, const double* src3, double* Rv) {
    try {
        Mesh mesh;
        mesh.build(c);
        CaseParams cp;
        cp.from_case(c);
        if (cp.solver != DAS_SOLVER_SIMPLEFOAM) throw std::runtime_error("a DASimpleFoam case expected");
        Options opt;
        if (!normalized) opt.s["normalizeResiduals"] = "TRes";
        const ResParams prm = make_params(cp, opt, 0);
        if (split && (prm.hasT || prm.mrf)) throw std::runtime_error("the face / cell split serves cases without a T field and MRF");
        DevMesh m = host_view(mesh);
        m.src3 = src3;
        const long long N = m.nC;
        const double* W = Win;
        std::vector<double> nut(N), gU(9 * N), gP(3 * N), gN(3 * N), gH(3 * N), rAU(N), HbyA(3 * N), q(m.nF);
        for (int k = 0; k < m.nC; k++) body_grad<double, false>(k, m, prm, W, nut.data(), gU.data(), gP.data(), gN.data(), gH.data());
        if (split) {
            std::vector<double> fc((size_t)DAS_FC_N * m.nIF), brec((size_t)DAS_BREC_N * (m.nF - m.nIF));
            for (int f = 0; f < m.nIF; f++) body_fcoef<double>(f, m, prm, W, nut.data(), gU.data(), gN.data(), fc.data());
            for (int b = 0; b < m.nF - m.nIF; b++) body_bcoef<double>(b, m, prm, W, nut.data(), gU.data(), brec.data());
            for (int k = 0; k < m.nC; k++) {  // SRC as eval_residual picks it: by the pointer
                if (src3) body_cell2<double, true>(k, m, prm, W, nut.data(), gU.data(), gP.data(), gN.data(), fc.data(), brec.data(), Rv, rAU.data(), HbyA.data());
                else body_cell2<double>(k, m, prm, W, nut.data(), gU.data(), gP.data(), gN.data(), fc.data(), brec.data(), Rv, rAU.data(), HbyA.data());
            }
        } else {
            for (int k = 0; k < m.nC; k++) {
                if (src3) body_cell<double, false, double, true>(k, m, prm, W, nut.data(), gU.data(), gP.data(), gN.data(), gH.data(), Rv, rAU.data(), HbyA.data());
                else body_cell<double, false, double>(k, m, prm, W, nut.data(), gU.data(), gP.data(), gN.data(), gH.data(), Rv, rAU.data(), HbyA.data());
            }
        }
        for (int f = 0; f < m.nF; f++) body_face<double, false>(f, m, prm, W, nut.data(), gP.data(), rAU.data(), HbyA.data(), q.data(), Rv);
        for (int k = 0; k < m.nC; k++) body_pres<double, false>(k, m, prm, q.data(), Rv);
        (void)n;
        return 0;
    } catch (const std::exception& e) {
        fprintf(stderr, "emu_ad_residual: %s\n", e.what());
        return -1;
    }
}
