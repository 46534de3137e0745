// TEST HARNESS ONLY (never linked into libdafoam_amd.so, never used by the product path).
// Runs the bodies the HIP kernels k_mq_metric / k_rn_terms / k_rn_seeds wrap (body_mesh_quality, rn_term, rn_seed,
// csrc/das_meshquality.hpp) in plain host loops, after the metric passes of csrc/das_geom.hpp in the same scalar type, so that the
// CPU-only test tier can check them against the numpy restatement (tests/test_mesh_quality_cpu.py).
#include <cstdio>
#include <stdexcept>
#include <vector>

#include "../../dafoam_amd/csrc/das_case.hpp"
#include "../../dafoam_amd/csrc/das_meshquality.hpp"

using namespace das;

template <class S>
static void metrics_on(const Mesh& m, const std::vector<S>& P, int metric, std::vector<S>& a) {
    const GeomTopo t = m.geom_topo();
    std::vector<FaceGeomT<S>> fg(m.nF);
    std::vector<CellGeomT<S>> cg(m.nC);
    for (int f = 0; f < m.nF; f++) geom_face<S>(f, t, P.data(), fg[f]);
    for (int c = 0; c < m.nC; c++)
        if (!geom_cell<S>(c, t, fg.data(), cg[c])) throw std::runtime_error("non-positive cell volume");
    a.resize(m.nF);
    for (int f = 0; f < m.nF; f++) a[f] = body_mesh_quality<S>(f, t, P.data(), fg.data(), cg.data(), metric);
}

// a[f] = body_mesh_quality<double> of every face of a bare polyhedral mesh at the points pts; with a point direction dX (3 nP) also
// da[f] = the tangent of body_mesh_quality<Dual<1>> along it
extern "C" int emu_mesh_quality(int nP, const double* pts, int nF, int nIF, int nC, const int* fptr, const int* fpts, const int* own, const int* nei,
                                int metric, const double* dX, double* a, double* da) {
    try {
        Mesh m;
        m.nP = nP; m.nF = nF; m.nIF = nIF; m.nC = nC; m.nPatch = 0;
        m.points.assign(pts, pts + 3LL * nP);
        m.face_ptr.assign(fptr, fptr + nF + 1);
        m.face_pts.assign(fpts, fpts + fptr[nF]);
        m.owner.assign(own, own + nF);
        m.neighbour.assign(nei, nei + nIF);
        m.bface_patch.assign(nF - nIF, 0);
        m.cyc_face.assign(nF - nIF, -1);
        m.bc.assign(1, PatchBC{});
        m.build_addressing();
        std::vector<double> av;
        metrics_on<double>(m, m.points, metric, av);
        for (int f = 0; f < nF; f++) a[f] = av[f];
        if (!dX) return 0;
        std::vector<Dual<1>> P(3LL * nP), ad;
        for (long long i = 0; i < 3LL * nP; i++) { P[i] = Dual<1>(pts[i]); P[i].d[0] = dX[i]; }
        metrics_on<Dual<1>>(m, P, metric, ad);
        for (int f = 0; f < nF; f++) da[f] = ad[f].d[0];
        return 0;
    } catch (const std::exception& e) {
        fprintf(stderr, "emu_mesh_quality: %s\n", e.what());
        return -1;
    }
}

// term[i] = rn_term, g[i] = coef rn_seed of row i for the residual vector R (n rows) and the block layout off / kind / w (nb blocks)
extern "C" int emu_residual_norm(long long n, const double* R, int nb, const long long* off, const int* kind, const double* w, long long nC, long long nF,
                                 long long nIF, int l1, double F, double coef, double* term, double* g) {
    if (nb > 8) return -1;
    RnRows r{};
    r.nb = nb;
    for (int b = 0; b < nb; b++) { r.off[b] = off[b]; r.kind[b] = kind[b]; r.w[b] = w[b]; }
    r.nC = nC; r.nF = nF; r.nIF = nIF; r.l1 = l1;
    for (long long i = 0; i < n; i++) { term[i] = rn_term(r, i, R[i]); g[i] = coef * rn_seed(r, i, R[i], F); }
    return 0;
}
