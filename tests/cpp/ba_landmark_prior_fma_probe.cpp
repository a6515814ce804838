// Compiled to ASSEMBLY, never run (tests/test_ba_landmark_prior_reference_cpu.py, tests/test_ba_landmark_prior_shim_cpu.py): the
// landmark prior's whitening must not be contracted into fused multiply-adds by a host compiler whose target has them (g++ -mfma
// contracts by default), or a host build would not give the device's bits where W r cancels.  Without PROBE_CERES: the maths of
// slam-tricks_amd/csrc/ba_landmark_prior.hpp; with it: ceres::LandmarkPriorFactor::Evaluate of include/stba/ceres.h.
#ifdef PROBE_CERES
#include "stba/ceres.h"
__attribute__((noinline)) bool probe(const double* pos, const double* w, const double* p, double* r, double* J) {
    stba_ceres::LandmarkPriorFactor f(pos, w);
    const double* prm[1] = {p};
    double* jac[1] = {J};
    return f.Evaluate(prm, r, jac);
}
#else
#include "../../slam-tricks_amd/csrc/ba_landmark_prior.hpp"
__attribute__((noinline)) void probe(const double* W, const double* pos, const double* p, double* out) {
    double rw[3];
    stba::lp_residual(W, pos, p, rw);
    for (int i = 0; i < 3; ++i) out[i] = rw[i];
    int e = 3;
    for (int a = 0; a < 3; ++a)
        for (int b = a; b < 3; ++b) out[e++] = stba::lp_wtw(W, a, b);
    for (int a = 0; a < 3; ++a) out[e++] = stba::lp_wtr(W, rw, a);
}
#endif
