// TEST HARNESS ONLY (never linked into libdafoam_amd.so, never used by the product path).
// Runs the vector form of the force body that the HIP kernel k_fc_face_force wraps (body_force_vec, csrc/das_kernels.hpp) in a plain
// host loop, next to the scalar body_force it was factored out of, so that the CPU-only test tier can check both against the numpy
// restatement (tests/test_force_coupling_cpu.py).
#include "../../dafoam_amd/csrc/das_case.hpp"

using namespace das;

template <bool RHO>
static void forces_on(const DevMesh& m, const ResParams& prm, const std::vector<double>& W, const int* faces, int nf, double pRef, const double* dir,
                      double* ff, double* fdot) {
    const long long N = m.nC;
    std::vector<double> nut(N), gU(9 * N), gP(3 * N), gN(3 * N), gH(3 * N), TU(3 * N);
    for (int c = 0; c < m.nC; c++) body_grad<double, RHO>(c, m, prm, W.data(), nut.data(), gU.data(), gP.data(), gN.data(), gH.data(), TU.data());
    for (int k = 0; k < nf; k++) {
        body_force_vec<double, RHO>(faces[k], m, prm, W.data(), nut.data(), gU.data(), pRef, ff + 3 * k);
        fdot[k] = body_force<double, RHO>(faces[k], m, prm, W.data(), nut.data(), gU.data(), dir + 3 * k, 1.0, pRef);
    }
}

// ff[3 k ..] = body_force_vec(faces[k]; pRef);  fdot[k] = body_force(faces[k]; dir[3 k ..], scale 1, pRef)
extern "C" int emu_face_forces(const das_case_t* c, const double* Win, long long n, const int* faces, int nf, double pRef, const double* dir, double* ff,
                               double* fdot) {
    try {
        Mesh mesh;
        mesh.build(c);
        CaseParams cp;
        cp.from_case(c);
        Options opt;
        const ResParams prm = make_params(cp, opt, 0);
        for (int k = 0; k < nf; k++)
            if (faces[k] < mesh.nIF || faces[k] >= mesh.nF) throw std::runtime_error("not a boundary face");
        std::vector<double> W(Win, Win + n);
        if (DAS_IS_COMPRESSIBLE(cp.solver)) forces_on<true>(host_view(mesh), prm, W, faces, nf, pRef, dir, ff, fdot);
        else forces_on<false>(host_view(mesh), prm, W, faces, nf, pRef, dir, ff, fdot);
        return 0;
    } catch (const std::exception& e) {
        fprintf(stderr, "emu_face_forces: %s\n", e.what());
        return -1;
    }
}
