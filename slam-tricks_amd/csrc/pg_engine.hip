// pg_engine.hip -- pose-graph SLAM on gfx950 (BASELINE config C4: 10k SE3 nodes, 40k relative-pose
// edges).  BUILD-DEFINED: the reference has no pose-graph code (SURVEY.md header fact 3); the
// conventions are the reference's Lie-group notes: right-multiplicative update T <- T exp(delta),
// tangent order [rho, theta] (st23-lie-group-v2/doc.tex:862-996, st21-lie/lie-group.tex:218-278),
// trajectory shape and ATE from st4-kalman/src/src/pose_simulation.cpp:17-88,198-209.
//
//   residual   r_ij = log(Z_ij^-1 T_i^-1 T_j)  in R^6
//   Jacobians  d r/d delta_j = Jr^-1(r),  d r/d delta_i = -Jr^-1(r) Ad(T_j^-1 T_i),
//              Jr^-1(r) = I + ad(r)/2 + ad(r)^2/12
//   solver     Levenberg-Marquardt (same control flow as the BA engine); the damped normal equations
//              (6 n_nodes unknowns, block-sparse) are solved matrix-free by preconditioned conjugate
//              gradients as an INEXACT Newton step: the PCG stops at |r| <= eta |g| with a forcing
//              sequence eta_k (Eisenstat-Walker), decided on the device.
//   preconditioner (round 4)  M^-1 = blockdiag(H_ii + D_i)^-1 + P (P^T (J^T J + D) P)^-1 P^T: two levels, additive.
//              The coarse space holds six rigid-body modes per GROUP of consecutive nodes (a stretch of
//              the trajectory moved as one body): delta_k = Ad(T_k^-1 T_ref(group)) xi.  Block Jacobi alone
//              leaves the long, smooth error modes of the chain (drift) to the Krylov iteration -- 939
//              iterations to 1e-12 at C4, the cap of 1000 on every LM iteration in round 3; a block
//              TRIDIAGONAL preconditioner (the odometry chain factored exactly) was measured first and
//              hardly helps (812: its diagonal carries the loop closures' stiffness, which the smooth
//              modes do not feel); the rigid-body coarse space cuts it to 67-109 (groups of 16-64
//              nodes), and with the forcing sequence a C4 LM iteration takes ~24 PCG iterations.
//              The coarse matrix (942 unknowns at C4) is inverted explicitly once per LM iteration
//              (dense_chol.hip, chol_spd_inverse_dev: the only MFMA work of this engine) and applied
//              as a dense product.
//
// Data in HBM: poses [n][7] (two copies), edges (i, j) int32, meas [m][7], r [m][6], Ji/Jj [36][m] (COMPONENT-major: entry k
// of edge e at k m + e, so that the lanes of a wave -- consecutive edges -- read and write consecutive addresses; edge-major
// [m][36] made every load instruction touch 64 cache lines: the matrix-free product took 24 us for 25 MB),
// g [6n], Hd [n][36] (diagonal blocks), Minv [n][36], PCG vectors x r z p q [6n].
#include <algorithm>
#include <atomic>
#include <chrono>
#include <cfloat>
#include <climits>
#include <cmath>
#include <functional>
#include <vector>

#include "ba_kernels.hpp"
#include "dd6.hpp"
#include "lm_policy.hpp"
#include "pg_covariance.hpp"
#include "pg_plan.hpp"
#include "robust_loss.hpp"

namespace stba {
namespace {

// ---------------------------------------------------------------- SE3 helpers (7-double poses)
__host__ __device__ inline void quat_mul7(const double* a, const double* b, double* o) {
    o[0] = a[3] * b[0] + a[0] * b[3] + a[1] * b[2] - a[2] * b[1];
    o[1] = a[3] * b[1] - a[0] * b[2] + a[1] * b[3] + a[2] * b[0];
    o[2] = a[3] * b[2] + a[0] * b[1] - a[1] * b[0] + a[2] * b[3];
    o[3] = a[3] * b[3] - a[0] * b[0] - a[1] * b[1] - a[2] * b[2];
}
__host__ __device__ inline void rot_vec(const double* q, const double* v, double* o) {
    double R[9];
    quat_to_rot(q, R);
    for (int i = 0; i < 3; ++i) o[i] = R[i * 3] * v[0] + R[i * 3 + 1] * v[1] + R[i * 3 + 2] * v[2];
}
__host__ __device__ inline void se3_compose(const double* a, const double* b, double* out) {
    double q[4], t[3];
    quat_mul7(a, b, q);
    rot_vec(a, b + 4, t);
    const double n = sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
    for (int i = 0; i < 4; ++i) out[i] = q[i] / n;
    for (int i = 0; i < 3; ++i) out[4 + i] = t[i] + a[4 + i];
}
__host__ __device__ inline void se3_inverse(const double* a, double* out) {
    const double qc[4] = {-a[0], -a[1], -a[2], a[3]};
    double t[3];
    rot_vec(qc, a + 4, t);
    for (int i = 0; i < 4; ++i) out[i] = qc[i];
    for (int i = 0; i < 3; ++i) out[4 + i] = -t[i];
}
__host__ __device__ inline void hat3d(const double* v, double* M) {
    M[0] = 0; M[1] = -v[2]; M[2] = v[1]; M[3] = v[2]; M[4] = 0; M[5] = -v[0]; M[6] = -v[1]; M[7] = v[0]; M[8] = 0;
}
// Sophus SE3::log of (q, t) -> [rho, theta]
__host__ __device__ inline void se3_log7(const double* T, double* xi) {
    const double n2 = T[0] * T[0] + T[1] * T[1] + T[2] * T[2], qw = T[3];
    double k;
    if (n2 < 1e-20) k = 2.0 / qw - (2.0 / 3.0) * n2 / (qw * qw * qw);
    else { const double n = sqrt(n2); k = 2.0 * ((qw < 0) ? atan2(-n, -qw) : atan2(n, qw)) / n; }
    const double w[3] = {k * T[0], k * T[1], k * T[2]};
    double V[9];
    so3_left_jacobian(w, V);
    // rho = V^-1 t
    const double aa = V[0], bb = V[1], cc = V[2], dd = V[3], ee = V[4], ff = V[5], gg = V[6], hh = V[7], ii = V[8];
    const double C0 = ee * ii - ff * hh, C1 = ff * gg - dd * ii, C2 = dd * hh - ee * gg;
    const double inv = 1.0 / (aa * C0 + bb * C1 + cc * C2);
    const double* t = T + 4;
    xi[0] = inv * (C0 * t[0] + (cc * hh - bb * ii) * t[1] + (bb * ff - cc * ee) * t[2]);
    xi[1] = inv * (C1 * t[0] + (aa * ii - cc * gg) * t[1] + (cc * dd - aa * ff) * t[2]);
    xi[2] = inv * (C2 * t[0] + (bb * gg - aa * hh) * t[1] + (aa * ee - bb * dd) * t[2]);
    xi[3] = w[0]; xi[4] = w[1]; xi[5] = w[2];
}
__host__ __device__ inline void se3_retract(const double* T, const double* d, double* out) {
    double e[7], R[9];
    so3_exp(d + 3, e);
    se3_exp_rt(d, R, e + 4);
    se3_compose(T, e, out);
}

// r, Ji, Jj of one edge
__device__ inline void pg_edge(const double* Ti, const double* Tj, const double* Z, double* r, double* Ji, double* Jj) {
    double Zi[7], Tii[7], A[7], E[7];
    se3_inverse(Z, Zi);
    se3_inverse(Ti, Tii);
    se3_compose(Tii, Tj, A);
    se3_compose(Zi, A, E);
    if (E[3] < 0) for (int k = 0; k < 4; ++k) E[k] = -E[k];
    se3_log7(E, r);
    if (!Ji) return;
    // Jr^-1 = I + ad/2 + ad^2/12, ad(xi) = [[hat(th), hat(rho)], [0, hat(th)]]
    double Hr[9], Ht[9], ad[36], Jr[36];
    hat3d(r, Hr); hat3d(r + 3, Ht);
    for (int k = 0; k < 36; ++k) ad[k] = 0.0;
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) { ad[i * 6 + j] = Ht[i * 3 + j]; ad[i * 6 + 3 + j] = Hr[i * 3 + j]; ad[(3 + i) * 6 + 3 + j] = Ht[i * 3 + j]; }
    for (int i = 0; i < 6; ++i)
        for (int j = 0; j < 6; ++j) {
            double s = 0.0;
            for (int k = 0; k < 6; ++k) s += ad[i * 6 + k] * ad[k * 6 + j];
            Jr[i * 6 + j] = (i == j ? 1.0 : 0.0) + 0.5 * ad[i * 6 + j] + s / 12.0;
        }
    for (int k = 0; k < 36; ++k) Jj[k] = Jr[k];
    // Ad(T_j^-1 T_i) = [[R, hat(t) R], [0, R]]
    double Ainv[7], R[9], Hh[9], AdM[36];
    se3_inverse(A, Ainv);
    quat_to_rot(Ainv, R);
    hat3d(Ainv + 4, Hh);
    for (int k = 0; k < 36; ++k) AdM[k] = 0.0;
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            double s = 0.0;
            for (int k = 0; k < 3; ++k) s += Hh[i * 3 + k] * R[k * 3 + j];
            AdM[i * 6 + j] = R[i * 3 + j]; AdM[i * 6 + 3 + j] = s; AdM[(3 + i) * 6 + 3 + j] = R[i * 3 + j];
        }
    for (int i = 0; i < 6; ++i)
        for (int j = 0; j < 6; ++j) {
            double s = 0.0;
            for (int k = 0; k < 6; ++k) s += Jr[i * 6 + k] * AdM[k * 6 + j];
            Ji[i * 6 + j] = -s;
        }
}

__device__ inline void block_sum2(double a, double b, double* out2) {
    __shared__ double s[2][4];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    for (int off = 32; off > 0; off >>= 1) { a += __shfl_down(a, off, 64); b += __shfl_down(b, off, 64); }
    if (lane == 0) { s[0][w] = a; s[1][w] = b; }
    __syncthreads();
    if (threadIdx.x == 0) { out2[0] = s[0][0] + s[0][1] + s[0][2] + s[0][3]; out2[1] = s[1][0] + s[1][1] + s[1][2] + s[1][3]; }
}

// device-resident scalars of one PCG solve; every kernel of iteration k reads rz[k & 1], the direction kernel writes rz[(k + 1) & 1]
struct PgPcgState {
    double rz[2];
    double rr0, rr, tol2;
    int iters, done, hit_cap, ticks;
};
// what the host polls (mapped, coherent host memory; written by workgroup 0 of the direction kernel, ticks last)
// what the launch-path PCG shows the polling host: a STAMPED block (common.hpp) of one line -- payload {rr0, rr, iters, done, hit_cap},
// stamp = the tick count
enum { PX_RR0 = 0, PX_RR = 1, PX_ITERS = 2, PX_DONE = 3, PX_HIT_CAP = 4, PX_COUNT = 5 };

// ---------------------------------------------------------------- kernels
// x <- W x for `cols` columns of a 6-row matrix held row-major with row stride `ld` (a 6-vector: cols = ld = 1): one column at a
// time through a 6-vector of temporaries, so that the product needs W (36) and six doubles on top of what is whitened in place
__device__ inline void pg_whiten_cols(const double* W, double* x, int cols, int ld) {
    for (int c = 0; c < cols; ++c) {
        double t[6];
        for (int a = 0; a < 6; ++a) {
            double s = 0.0;
            for (int k = 0; k < 6; ++k) s += W[a * 6 + k] * x[k * ld + c];
            t[a] = s;
        }
        for (int a = 0; a < 6; ++a) x[a * ld + c] = t[a];
    }
}

// J <- sqrt(rho') (J - k r (r^T J)) for the 6 x 6 row-major J of one edge end, one column at a time (k = alpha / s of Ceres' corrector;
// k == 0: the scaling alone)
__device__ inline void pg_correct_cols(const double* re, double* J, double sq, double k) {
    for (int c = 0; c < 6; ++c) {
        if (k != 0.0) {
            double t = 0.0;
            for (int a = 0; a < 6; ++a) t += re[a] * J[a * 6 + c];
            t *= k;
            for (int a = 0; a < 6; ++a) J[a * 6 + c] = sq * (J[a * 6 + c] - re[a] * t);
        } else {
            for (int a = 0; a < 6; ++a) J[a * 6 + c] = sq * J[a * 6 + c];
        }
    }
}

// INFO = false: every edge weighted by the identity -- the kernel as it was before edges had information matrices; Winfo is not
// read.  INFO = true: the residual and both Jacobians are whitened by the edge's square-root information W_e (Winfo[k * n_edges + e],
// laid out like Ji) right behind pg_edge: cost, stores, the constant-node zeroing and the contrib block below all see W r, W Ji,
// W Jj, and so does every consumer of what this kernel writes.  Two instantiations and not a runtime branch: an engine without
// weights runs the instruction stream it ran before.
// ROBUST = false: no edge has a loss, the kernel as it was before (lkind, la, lb, lscale are not read).  ROBUST = true: behind the
// whitening the edge's loss (lkind[e], la[e], lb[e], lscale[e]: read by edge index) is evaluated at s = |r|^2 and Ceres' corrector
// turns r and both Jacobians into r', J' with J'^T r' = rho' J^T r and J'^T J' the Triggs approximation of the robustified Hessian;
// the edge's cost term is rho(s).  Every store and the contrib block see r', J'.  An edge of kind TRIVIAL and scale 1 is left alone:
// what it stores compares == to the ROBUST = false kernel's.  The kind is a runtime switch: lanes of a wave may differ.
template <bool INFO, bool ROBUST>
__global__ __launch_bounds__(256) void pg_linearize_kernel(int n_edges, const double* __restrict__ poses,
                                                           const int* __restrict__ ei, const int* __restrict__ ej,
                                                           const double* __restrict__ meas,
                                                           const unsigned char* __restrict__ fixed, int with_jac,
                                                           double* __restrict__ r, double* __restrict__ Ji,
                                                           double* __restrict__ Jj, double* __restrict__ partial,
                                                           double* __restrict__ contrib, const double* __restrict__ Winfo,
                                                           const int* __restrict__ lkind, const double* __restrict__ la,
                                                           const double* __restrict__ lb, const double* __restrict__ lscale) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    double c = 0.0;
    if (e < n_edges) {
        const int i = ei[e], j = ej[e];
        double Ti[7], Tj[7], Z[7], re[6], ji[36], jj[36];
        for (int k = 0; k < 7; ++k) { Ti[k] = poses[(size_t)i * 7 + k]; Tj[k] = poses[(size_t)j * 7 + k]; Z[k] = meas[(size_t)e * 7 + k]; }
        pg_edge(Ti, Tj, Z, re, with_jac ? ji : nullptr, jj);
        if (INFO) {
            double We[36];
            for (int k = 0; k < 36; ++k) We[k] = Winfo[(size_t)k * n_edges + e];
            pg_whiten_cols(We, re, 1, 1);
            if (with_jac) { pg_whiten_cols(We, ji, 6, 6); pg_whiten_cols(We, jj, 6, 6); }
        }
        for (int k = 0; k < 6; ++k) c += re[k] * re[k];
        if (ROBUST) {
            const int kind = lkind[e];
            const double sc = lscale[e];
            if (kind != STBA_LOSS_TRIVIAL || sc != 1.0) {
                const double s = c;
                double rho[3];
                robust_loss(kind, la[e], lb[e], s, rho);
                for (int k = 0; k < 3; ++k) rho[k] *= sc;
                c = rho[0];
                const double sq = sqrt(rho[1]);
                double rs = sq, ak = 0.0;                     // residual scaling, alpha / s
                if (s != 0.0 && rho[2] > 0.0) {
                    const double alpha = 1.0 - sqrt(1.0 + 2.0 * s * rho[2] / rho[1]);
                    rs = sq / (1.0 - alpha);
                    ak = alpha / s;
                }
                if (with_jac) { pg_correct_cols(re, ji, sq, ak); pg_correct_cols(re, jj, sq, ak); }
                for (int k = 0; k < 6; ++k) re[k] *= rs;
            }
        }
        if (r) for (int k = 0; k < 6; ++k) r[(size_t)e * 6 + k] = re[k];
        if (with_jac) {
            const bool fi = fixed && fixed[i], fj = fixed && fixed[j];
            for (int k = 0; k < 36; ++k) { ji[k] = fi ? 0.0 : ji[k]; jj[k] = fj ? 0.0 : jj[k]; Ji[(size_t)k * n_edges + e] = ji[k]; Jj[(size_t)k * n_edges + e] = jj[k]; }
            // what this edge adds to its two nodes' gradient and diagonal block, 27 doubles per end {J^T r (6), upper triangle of J^T J (21)}:
            // pg_gather_blocks_kernel sums a node's ends in a fixed order -- no atomics (the scatter with 42 FP64 atomics per edge
            // end took 156 us per linearisation at C4, 9 % of an LM iteration; rocprofv3, profiles/r4_b_c4_kernel_stats.csv)
            if (contrib) {
                for (int side = 0; side < 2; ++side) {
                    const double* J = side ? jj : ji;
                    double* out = contrib + ((size_t)e * 2 + side) * 28;
                    int w = 0;
                    for (int a = 0; a < 6; ++a) {
                        double sg = 0.0;
                        for (int k = 0; k < 6; ++k) sg += J[k * 6 + a] * re[k];
                        out[w++] = sg;
                    }
                    for (int a = 0; a < 6; ++a)
                        for (int b = a; b < 6; ++b) {
                            double h = 0.0;
                            for (int k = 0; k < 6; ++k) h += J[k * 6 + a] * J[k * 6 + b];
                            out[w++] = h;
                        }
                    out[27] = 0.0;
                }
            }
        }
    }
    double out2[2];
    block_sum2(c, 0.0, out2);
    if (threadIdx.x == 0) partial[blockIdx.x] = out2[0];
}

// ---- per-edge weights: what the caller gives ([m][36] row-major) -> the component-major array the linearisation reads
// One edge per lane.  sqrt_form = 0: `in` holds an information matrix Omega_e (symmetric positive definite; the lower triangle is
// factored), Omega = L L^T by an unblocked Cholesky in double-double, W_e = L^T rounded to FP64 (information6_factor, dd6.hpp: the
// one the bundle adjustment's factor setters call on the host).  sqrt_form = 1: `in` holds W_e itself, which is only transposed into
// the component-major array.  A non-finite entry anywhere in the 36, or a pivot that is not a positive finite number, refuses the
// edge: the smallest such edge index ends up in *bad (which the host set to INT_MAX), and the host throws the whole array away.
__global__ __launch_bounds__(256) void pg_information_kernel(int n_edges, const double* __restrict__ in, int sqrt_form,
                                                             double* __restrict__ Wout, int* __restrict__ bad) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= n_edges) return;
    double A[36];
    bool ok = true;
    for (int k = 0; k < 36; ++k) { A[k] = in[(size_t)e * 36 + k]; ok = ok && isfinite(A[k]); }
    double Wl[36];
    if (sqrt_form) {
        for (int k = 0; k < 36; ++k) Wl[k] = A[k];
    } else {
        ok = ok && information6_factor(A, Wl);
    }
    if (!ok) { atomicMin(bad, e); return; }
    for (int k = 0; k < 36; ++k) Wout[(size_t)k * n_edges + e] = Wl[k];
}

// gradient and diagonal blocks: g_i += Ji^T r, Hd_i += Ji^T Ji (same for j), FP64 atomics
__global__ __launch_bounds__(256) void pg_accumulate_kernel(int n_edges, const int* __restrict__ ei, const int* __restrict__ ej,
                                                            const double* __restrict__ r, const double* __restrict__ Ji,
                                                            const double* __restrict__ Jj, double* __restrict__ g,
                                                            double* __restrict__ Hd) {
    const int gid = blockIdx.x * 256 + threadIdx.x;
    const int e = gid >> 1, side = gid & 1;
    if (e >= n_edges) return;
    const int node = side ? ej[e] : ei[e];
    const double* J = (side ? Jj : Ji) + e;
    const double* re = r + (size_t)e * 6;
    double Jl[36], rl[6];
    bool any = false;
    for (int k = 0; k < 36; ++k) { Jl[k] = J[(size_t)k * n_edges]; any |= (Jl[k] != 0.0); }
    if (!any) return;   // constant node
    for (int k = 0; k < 6; ++k) rl[k] = re[k];
    for (int a = 0; a < 6; ++a) {
        double s = 0.0;
        for (int k = 0; k < 6; ++k) s += Jl[k * 6 + a] * rl[k];
        unsafeAtomicAdd(&g[(size_t)node * 6 + a], s);
        for (int b = 0; b <= a; ++b) {
            double h = 0.0;
            for (int k = 0; k < 6; ++k) h += Jl[k * 6 + a] * Jl[k * 6 + b];
            unsafeAtomicAdd(&Hd[(size_t)node * 36 + a * 6 + b], h);
            if (b != a) unsafeAtomicAdd(&Hd[(size_t)node * 36 + b * 6 + a], h);
        }
    }
}

// LM diagonal + block-Jacobi preconditioner M_i = (Hd_i + diag(d_i))^-1 (6x6 Gauss-Jordan on an SPD block)
__global__ __launch_bounds__(256) void pg_precond_kernel(int n_nodes, const double* __restrict__ Hd, double* __restrict__ scale,
                                                         int init_scale, int use_scaling, double radius, double dmin, double dmax,
                                                         const unsigned char* __restrict__ fixed, double* __restrict__ d,
                                                         double* __restrict__ Minv) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n_nodes) return;
    double A[36], B[36];
    for (int k = 0; k < 36; ++k) { A[k] = Hd[(size_t)i * 36 + k]; B[k] = 0.0; }
    const bool fx = fixed && fixed[i];
    for (int a = 0; a < 6; ++a) {
        const double h = A[a * 7];
        double s = 1.0;
        if (use_scaling) { if (init_scale) { s = 1.0 / (1.0 + sqrt(h)); scale[(size_t)i * 6 + a] = s; } else s = scale[(size_t)i * 6 + a]; }
        else if (init_scale) scale[(size_t)i * 6 + a] = 1.0;
        const double s2 = s * s;
        const double dv = fmin(fmax(h * s2, dmin), dmax) / radius / s2;
        d[(size_t)i * 6 + a] = dv;
        A[a * 7] += dv;
        B[a * 7] = 1.0;
    }
    if (fx) { for (int k = 0; k < 36; ++k) Minv[(size_t)i * 36 + k] = 0.0; return; }
    for (int c = 0; c < 6; ++c) {          // Gauss-Jordan without pivoting (SPD + damping)
        const double inv = 1.0 / A[c * 7];
        for (int k = 0; k < 6; ++k) { A[c * 6 + k] *= inv; B[c * 6 + k] *= inv; }
        for (int rr = 0; rr < 6; ++rr) {
            if (rr == c) continue;
            const double f = A[rr * 6 + c];
            for (int k = 0; k < 6; ++k) { A[rr * 6 + k] -= f * A[c * 6 + k]; B[rr * 6 + k] -= f * B[c * 6 + k]; }
        }
    }
    for (int k = 0; k < 36; ++k) Minv[(size_t)i * 36 + k] = B[k];
}

// q = D p   (then the edge kernel adds J^T J p)
__global__ __launch_bounds__(256) void pg_diag_mul_kernel(int n, const double* __restrict__ d, const double* __restrict__ p,
                                                          double* __restrict__ q, int use_d) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) q[i] = use_d ? d[i] * p[i] : 0.0;
}

__global__ __launch_bounds__(256) void pg_matvec_kernel(int n_edges, const int* __restrict__ ei, const int* __restrict__ ej,
                                                        const double* __restrict__ Ji, const double* __restrict__ Jj,
                                                        const double* __restrict__ p, double* __restrict__ q) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= n_edges) return;
    const int i = ei[e], j = ej[e];
    double A[36], B[36];
    for (int k = 0; k < 36; ++k) { A[k] = Ji[(size_t)k * n_edges + e]; B[k] = Jj[(size_t)k * n_edges + e]; }
    double pi[6], pj[6], t[6];
    for (int k = 0; k < 6; ++k) { pi[k] = p[(size_t)i * 6 + k]; pj[k] = p[(size_t)j * 6 + k]; }
    for (int a = 0; a < 6; ++a) {
        double s = 0.0;
        for (int k = 0; k < 6; ++k) s += A[a * 6 + k] * pi[k] + B[a * 6 + k] * pj[k];
        t[a] = s;
    }
    for (int k = 0; k < 6; ++k) {
        double si = 0.0, sj = 0.0;
        for (int a = 0; a < 6; ++a) { si += A[a * 6 + k] * t[a]; sj += B[a * 6 + k] * t[a]; }
        if (si != 0.0) unsafeAtomicAdd(&q[(size_t)i * 6 + k], si);
        if (sj != 0.0) unsafeAtomicAdd(&q[(size_t)j * 6 + k], sj);
    }
}

// partial[b] = {dot(a, b2), dot(a, a)}
__global__ __launch_bounds__(256) void pg_dot_kernel(int n, const double* __restrict__ a, const double* __restrict__ b2,
                                                     double* __restrict__ partial) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    double x = 0.0, y = 0.0;
    if (i < n) { x = a[i] * b2[i]; y = a[i] * a[i]; }
    double out2[2];
    block_sum2(x, y, out2);
    if (threadIdx.x == 0) { partial[blockIdx.x * 2] = out2[0]; partial[blockIdx.x * 2 + 1] = out2[1]; }
}

// sum of nb per-workgroup partials, by the WHOLE workgroup (256 threads): a strided share per thread, a shuffle tree per
// wave, the four waves in order -- the same order in every workgroup and on every rank, so every one of them gets the same
// bits.  (Every thread summing all partials serially -- 275 dependent loads -- made pg_pcg_update_kernel 27.5 us long, 40 %
// of a PCG iteration: profiles/r3_a_c4_kernel_stats.csv.)
__device__ inline double sum_partials_dev(const double* partial, int nb, int stride, int off) {
    __shared__ double s_w[4];
    __shared__ double s_tot;
    double v = 0.0;
    for (int k = threadIdx.x; k < nb; k += 256) v += partial[k * stride + off];
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    __syncthreads();                                     // (the shared slots may still be read from a previous call)
    if ((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0) s_tot = (s_w[0] + s_w[1]) + (s_w[2] + s_w[3]);
    __syncthreads();
    return s_tot;
}

// ---------------------------------------------------------------- one rank: a PCG iteration in THREE launches, no atomics
// (1) p^T q = p^T D p + |J p|^2 = sum_i d_i p_i^2 + sum_e |t_e|^2 with t_e = J_e [p_i; p_j]: the dot product needs no pass over
//     the finished q -- the edge kernel adds up |t_e|^2, the kernel that makes the direction p adds up d p^2.
// (2) q is never scattered: the edge kernel stores u_e = (Ji^T t_e | Jj^T t_e), 12 doubles per edge, component-major, and the
//     node kernel GATHERS q_i = d_i p_i + sum over the node's edge ends of u (a CSR of the ends built at create time) while it
//     updates x, r, z.  The scatter with FP64 atomics was the bound of the product: 480 k device-scope atomics per product
//     retire at ~20 G/s whatever the access pattern -- the product scaled linearly with the edge count at 1.65 G edges/s
//     (24.7 us at 40 k edges, 95 us at 160 k, 387 us at 640 k).  Measured on the way: one lane per edge END with a segmented
//     scan over a node's lanes and 6 atomics per node instead of 12 per edge (21.1 against 23.8 us: fewer atomics, but every
//     edge read twice and no coalescing); the whole loop as ONE persistent kernel with four grid barriers per iteration
//     (correct, 59 us per iteration against 40 us for the launches: a barrier across eight XCDs costs more than a kernel
//     boundary).
//     (Also measured: the direction p = z + beta p_old formed on the fly by the edge kernel and again by the node kernel, the
//     node term of the dot product added up by the edge ends -- TWO launches per iteration: 32 us against 30 us for three.
//     Every kernel that needs a scalar of the loop adds up its partial sums first, ~2 us each; two kernels that need three
//     each lose more than the launch they save.)
__global__ __launch_bounds__(256) void pg_edge_product_kernel(int n_edges, const int* __restrict__ ei, const int* __restrict__ ej,
                                                              const double* __restrict__ Ji, const double* __restrict__ Jj,
                                                              const double* __restrict__ p, double* __restrict__ u,
                                                              double* __restrict__ part_tt, const PgPcgState* __restrict__ state) {
    if (state && state->done) return;          // (the solve has converged: see pg_pcg_dir4_kernel)
    const int e = blockIdx.x * 256 + threadIdx.x;
    double tt2 = 0.0;
    if (e < n_edges) {
        const int i = ei[e], j = ej[e];
        double A[36], B[36];
        for (int k = 0; k < 36; ++k) { A[k] = Ji[(size_t)k * n_edges + e]; B[k] = Jj[(size_t)k * n_edges + e]; }
        double pi[6], pj[6], t[6];
        for (int k = 0; k < 6; ++k) { pi[k] = p[(size_t)i * 6 + k]; pj[k] = p[(size_t)j * 6 + k]; }
        for (int a = 0; a < 6; ++a) {
            double s = 0.0;
            for (int k = 0; k < 6; ++k) s += A[a * 6 + k] * pi[k] + B[a * 6 + k] * pj[k];
            t[a] = s;
            tt2 += s * s;
        }
        // u edge-major, 12 doubles per edge (i-side | j-side): the node kernel's gather then reads 48 contiguous bytes per edge end
        // (component-major u -- better for these stores -- made it six scattered 8-byte loads per end: 14 us for the node kernel)
        double ue[12];
        for (int k = 0; k < 6; ++k) {
            double si = 0.0, sj = 0.0;
            for (int a = 0; a < 6; ++a) { si += A[a * 6 + k] * t[a]; sj += B[a * 6 + k] * t[a]; }
            ue[k] = si; ue[6 + k] = sj;
        }
        double2* dst = reinterpret_cast<double2*>(u + (size_t)e * 12);
        for (int k = 0; k < 6; ++k) dst[k] = make_double2(ue[2 * k], ue[2 * k + 1]);
    }
    double out2[2];
    block_sum2(tt2, 0.0, out2);
    if (threadIdx.x == 0) { part_tt[blockIdx.x * 2] = out2[0]; part_tt[blockIdx.x * 2 + 1] = 0.0; }
}

// ================================================================= round 4: two-level preconditioner, device-side PCG control
// (PG_NT = 1024 threads = PG_NPW = 128 nodes x 8 lanes: pg_plan.hpp)

// sum of nb per-workgroup partials by a workgroup of NT threads, fixed order (same bits in every workgroup and on every rank)
template <int NT>
__device__ inline double sum_partials_n(const double* partial, int nb, int stride, int off) {
    __shared__ double s_w[NT / 64];
    __shared__ double s_tot;
    double v = 0.0;
    for (int k = threadIdx.x; k < nb; k += NT) v += partial[k * stride + off];
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0) { double t = 0.0; for (int w = 0; w < NT / 64; ++w) t += s_w[w]; s_tot = t; }
    __syncthreads();
    return s_tot;
}
template <int NT>
__device__ inline void block_sum2_n(double a, double b, double* out2) {
    __shared__ double s[2][NT / 64];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    for (int off = 32; off > 0; off >>= 1) { a += __shfl_down(a, off, 64); b += __shfl_down(b, off, 64); }
    __syncthreads();
    if (lane == 0) { s[0][w] = a; s[1][w] = b; }
    __syncthreads();
    if (threadIdx.x == 0) {
        double x = 0.0, y = 0.0;
        for (int k = 0; k < NT / 64; ++k) { x += s[0][k]; y += s[1][k]; }
        out2[0] = x; out2[1] = y;
    }
}

// gradient and diagonal blocks of a node = sum over its edge ends of the 27 doubles the linearise kernel left per end (fixed order: no
// atomics, same bits every run).  Eight lanes per node, one end each per trip, a butterfly over the eight lanes.
__global__ __launch_bounds__(PG_NT) void pg_gather_blocks_kernel(int n, const int* __restrict__ node_start, const int* __restrict__ end_code,
                                                                const double* __restrict__ contrib, double* __restrict__ g, double* __restrict__ Hd) {
    const int t = threadIdx.x, nl = t >> 3, k = t & 7;
    const int node = blockIdx.x * PG_NPW + nl;
    double acc[27];
    for (int q = 0; q < 27; ++q) acc[q] = 0.0;
    if (node < n) {
        const int e1 = node_start[node + 1];
        for (int c = node_start[node] + k; c < e1; c += 8) {
            const double2* src = reinterpret_cast<const double2*>(contrib + (size_t)end_code[c] * 28);
            for (int q = 0; q < 13; ++q) { const double2 v = src[q]; acc[2 * q] += v.x; acc[2 * q + 1] += v.y; }
            acc[26] += src[13].x;
        }
    }
    for (int q = 0; q < 27; ++q) {
        acc[q] += __shfl_xor(acc[q], 1, 8);
        acc[q] += __shfl_xor(acc[q], 2, 8);
        acc[q] += __shfl_xor(acc[q], 4, 8);
    }
    if (node < n && k < 6) {
        // row k of the symmetric block from the packed upper triangle: entry (a, b), a <= b, at 6 + a (13 - a) / 2 + (b - a)
        double gk = 0.0, row[6];
        for (int a = 0; a < 6; ++a) if (a == k) gk = acc[a];
        for (int b = 0; b < 6; ++b) {
            double v = 0.0;
            for (int a = 0; a < 6; ++a) {
                const int lo = a < b ? a : b, hi = a < b ? b : a;
                if (a == k) v = acc[6 + lo * (13 - lo) / 2 + (hi - lo)];
            }
            row[b] = v;
        }
        g[(size_t)node * 6 + k] = gk;
        for (int b = 0; b < 6; ++b) Hd[(size_t)node * 36 + k * 6 + b] = row[b];
    }
}

// |g|^2 and |g|_inf as per-workgroup partials {sum, max} (behind the cross-rank sum of g when there are several ranks)
__global__ __launch_bounds__(256) void pg_gnorm_kernel(int N, const double* __restrict__ g, double* __restrict__ part) {
    __shared__ double sm[4];
    const int i = blockIdx.x * 256 + threadIdx.x;
    const double v = i < N ? g[i] : 0.0;
    double s = v * v, mx = fabs(v);
    for (int o = 32; o > 0; o >>= 1) { s += __shfl_down(s, o, 64); mx = fmax(mx, __shfl_down(mx, o, 64)); }
    __shared__ double ss[4];
    if ((threadIdx.x & 63) == 0) { ss[threadIdx.x >> 6] = s; sm[threadIdx.x >> 6] = mx; }
    __syncthreads();
    if (threadIdx.x == 0) { part[blockIdx.x * 2] = (ss[0] + ss[1]) + (ss[2] + ss[3]); part[blockIdx.x * 2 + 1] = fmax(fmax(sm[0], sm[1]), fmax(sm[2], sm[3])); }
}

// damping term of the coarse matrix: Dc[group] = sum over the group's nodes of P_k^T diag(d_k) P_k (6 x 6), one workgroup per group
__global__ __launch_bounds__(256) void pg_coarse_dc_kernel(int n, int agg, const double* __restrict__ AdP, const double* __restrict__ d,
                                                           double* __restrict__ Dc) {
    __shared__ double sw[4][36];
    const int a = blockIdx.x, t = threadIdx.x;
    const int k0 = a * agg, k1 = min(n, k0 + agg);
    double acc[36];
    for (int q = 0; q < 36; ++q) acc[q] = 0.0;
    for (int item = t; item < (k1 - k0) * 6; item += 256) {          // (node, tangent component)
        const int k = k0 + item / 6, c = item % 6;
        const double dv = d[(size_t)k * 6 + c];
        double row[6];
        for (int u = 0; u < 6; ++u) row[u] = AdP[(size_t)k * 36 + c * 6 + u];
        for (int u = 0; u < 6; ++u)
            for (int w = 0; w < 6; ++w) acc[u * 6 + w] += row[u] * dv * row[w];
    }
    for (int q = 0; q < 36; ++q) {
        double v = acc[q];
        for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
        if ((t & 63) == 0) sw[t >> 6][q] = v;
    }
    __syncthreads();
    if (t < 36) Dc[(size_t)a * 36 + t] = (sw[0][t] + sw[1][t]) + (sw[2][t] + sw[3][t]);
}

// coarse basis: P_k = Ad(T_k^-1 T_ref), T_ref = the pose in the middle of the node's group; zero for constant nodes.
// Ad(R, t) = [[R, hat(t) R], [0, R]] for the tangent order [rho, theta] (st23-lie-group-v2/doc.tex:945-963)
__global__ __launch_bounds__(256) void pg_coarse_basis_kernel(int n, int agg, const double* __restrict__ poses,
                                                              const unsigned char* __restrict__ fixed, double* __restrict__ AdP) {
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k >= n) return;
    double M[36];
    for (int q = 0; q < 36; ++q) M[q] = 0.0;
    if (!(fixed && fixed[k])) {
        const int ref = min((k / agg) * agg + agg / 2, n - 1);
        double Tk[7], Tr[7], Tki[7], rel[7], R[9], Hh[9];
        for (int q = 0; q < 7; ++q) { Tk[q] = poses[(size_t)k * 7 + q]; Tr[q] = poses[(size_t)ref * 7 + q]; }
        se3_inverse(Tk, Tki);
        se3_compose(Tki, Tr, rel);
        quat_to_rot(rel, R);
        hat3d(rel + 4, Hh);
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 3; ++j) {
                double s = 0.0;
                for (int q = 0; q < 3; ++q) s += Hh[i * 3 + q] * R[q * 3 + j];
                M[i * 6 + j] = R[i * 3 + j]; M[i * 6 + 3 + j] = s; M[(3 + i) * 6 + 3 + j] = R[i * 3 + j];
            }
    }
    for (int q = 0; q < 36; ++q) AdP[(size_t)k * 36 + q] = M[q];
}

// Galerkin coarse matrix without the damping term, Ac0 = P^T J^T J P (nc x nc, dense): one workgroup per group of nodes
// = six rows of Ac0, from the ASSEMBLED blocks (round 5; until then every edge end re-made G = J P from two scattered Jacobians, 71 us):
//   the diagonal block of the group gets  sum over its nodes of P_i^T Hd_i P_i  (Hd_i = the node's diagonal block of J^T J, which
//   the linearisation leaves) and, for every edge end whose other node lies in the same group, P_s^T B P_o;
//   block (group, group of the other node) gets P_s^T B P_o for every other end -- B = J_s^T J_o is the end's block of
//   pg_offdiag_kernel, read coalesced in CSR order.  The other end does the same from its side, so the four blocks of an edge are
//   all made and no workgroup writes another one's rows.
// The row panel is accumulated in LDS and written once, zeros included: no global atomics, no memset.
// REPRODUCIBLE sums (round 5; until then the four waves added to the panel in arrival order and the preconditioner -- hence every
// PCG iterate -- differed in the last bits from run to run): every block of the panel is added to by ONE wave, the wave
// (other group) mod 4, whose adds meet an LDS address in program and lane order.  Each wave first collects ITS ends, in CSR order,
// into a list of its own (ballot + prefix count), then works through the list with all lanes.
// Several ranks (edge shards): Hd is the cross-rank sum, so only rank 0 adds the nodes' term (add_nodes).
__global__ __launch_bounds__(256) void pg_coarse_build_kernel(int n, int agg, int nc, int add_nodes, const int* __restrict__ node_start,
                                                              const int* __restrict__ end_node, const int* __restrict__ end_rem,
                                                              const double* __restrict__ Bend, const double* __restrict__ Hd,
                                                              const double* __restrict__ AdP, double* __restrict__ Ac0) {
    extern __shared__ double rowp[];            // [6][nc] | four lists of edge ends (int)
    __shared__ double dgp[4][36];
    __shared__ double dnode[64][37];
    const int a = blockIdx.x, t = threadIdx.x, lane = t & 63, wv = t >> 6;
    for (int q = t; q < 6 * nc; q += 256) rowp[q] = 0.0;
    const int k0 = a * agg, k1 = min(n, k0 + agg);
    const int c0 = node_start[k0], c1 = node_start[k1];
    const size_t m2 = (size_t)node_start[n];
    int* mylist = reinterpret_cast<int*>(rowp + (size_t)6 * nc) + (size_t)wv * (c1 - c0);
    int cnt = 0;
    for (int cb = c0; cb < c1; cb += 64) {
        const int c = cb + lane;
        const bool mine = c < c1 && ((end_rem[c] / agg) & 3) == wv;
        const unsigned long long bal = __ballot(mine);
        if (mine) mylist[cnt + __popcll(bal & ((1ull << lane) - 1ull))] = c;
        cnt += __popcll(bal);
    }
    // the nodes' term: one node per thread (groups of more than 64 nodes: in rounds), summed over the nodes in order below
    double dsum = 0.0;                          // thread q < 36: entry q of the diagonal block
    for (int base = k0; base < k1; base += 64) {
        __syncthreads();
        const int node = base + t;
        if (t < 64) {
            double M[36];
            for (int q = 0; q < 36; ++q) M[q] = 0.0;
            if (node < k1 && add_nodes) {
                double H[36], P[36], T[36];
                for (int q = 0; q < 36; ++q) { H[q] = Hd[(size_t)node * 36 + q]; P[q] = AdP[(size_t)node * 36 + q]; }
                for (int i = 0; i < 6; ++i)
                    for (int j = 0; j < 6; ++j) {
                        double s2 = 0.0;
                        for (int q = 0; q < 6; ++q) s2 += H[i * 6 + q] * P[q * 6 + j];
                        T[i * 6 + j] = s2;
                    }
                for (int u = 0; u < 6; ++u)
                    for (int v = 0; v < 6; ++v) {
                        double s2 = 0.0;
                        for (int q = 0; q < 6; ++q) s2 += P[q * 6 + u] * T[q * 6 + v];
                        M[u * 6 + v] = s2;
                    }
            }
            for (int q = 0; q < 36; ++q) dnode[t][q] = M[q];
        }
        __syncthreads();
        if (t < 36) for (int i = 0; i < 64; ++i) dsum += dnode[i][t];
    }
    __syncthreads();
    double dg[36];
    for (int q = 0; q < 36; ++q) dg[q] = 0.0;
    for (int idx = lane; idx < cnt; idx += 64) {
        const int c = mylist[idx];
        const int self = end_node[c], other = end_rem[c];
        double B[36], P[36], T[36];
        for (int q = 0; q < 36; ++q) { B[q] = Bend[(size_t)q * m2 + c]; P[q] = AdP[(size_t)other * 36 + q]; }
        for (int i = 0; i < 6; ++i)               // T = B P_o
            for (int j = 0; j < 6; ++j) {
                double s2 = 0.0;
                for (int q = 0; q < 6; ++q) s2 += B[i * 6 + q] * P[q * 6 + j];
                T[i * 6 + j] = s2;
            }
        for (int q = 0; q < 36; ++q) P[q] = AdP[(size_t)self * 36 + q];
        const int ao = other / agg;
        for (int u = 0; u < 6; ++u)
            for (int v = 0; v < 6; ++v) {
                double so = 0.0;
                for (int q = 0; q < 6; ++q) so += P[q * 6 + u] * T[q * 6 + v];
                if (ao == a) dg[u * 6 + v] += so;
                else unsafeAtomicAdd(&rowp[u * nc + 6 * ao + v], so);
            }
    }
    // the diagonal block: the waves' register sums through a shuffle tree each, the four waves in order, then the nodes' term
    for (int q = 0; q < 36; ++q) {
        double v = dg[q];
        for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
        if (lane == 0) dgp[wv][q] = v;
    }
    __syncthreads();
    if (t < 36) rowp[(t / 6) * nc + 6 * a + (t % 6)] = ((dgp[0][t] + dgp[1][t]) + (dgp[2][t] + dgp[3][t])) + dsum;
    __syncthreads();
    for (int q = t; q < 6 * nc; q += 256) Ac0[(size_t)(6 * a + q / nc) * nc + (q % nc)] = rowp[q];
}

// the inversion workspace of an LM iteration: W = [Ac0 + P^T D P (identity-padded to np) | . ; I | 0], see chol_spd_inverse_dev
__global__ __launch_bounds__(256) void pg_coarse_assemble_kernel(int nc, int np, const double* __restrict__ Ac0,
                                                                 const double* __restrict__ Dc, double* __restrict__ W) {
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    const size_t per = (size_t)np * np;
    if (idx >= 3 * per) return;
    const int quad = (int)(idx / per);
    const int r = (int)((idx % per) / np), c = (int)(idx % np);
    const size_t ldw = 2 * (size_t)np;
    if (quad == 1) { W[(np + r) * ldw + c] = (r == c) ? 1.0 : 0.0; return; }
    if (quad == 2) { W[(np + r) * ldw + np + c] = 0.0; return; }
    double v = (r == c) ? 1.0 : 0.0;
    if (r < nc && c < nc) {
        v = Ac0[(size_t)r * nc + c];
        if (r / 6 == c / 6) {
            v += Dc[(size_t)(r / 6) * 36 + (r % 6) * 6 + (c % 6)];
            if (r == c && !(v > 0.0)) v = 1.0;          // a group of constant nodes
        }
    }
    W[r * ldw + c] = v;
}

// Ainv = -(lower right block of W), symmetric, full.  cflag: the pivot flag of the partial factorisation that made W -- a non-positive
// pivot (or a NaN) in P^T (J^T J + D) P leaves garbage there: the coarse correction is then switched OFF for this operator (Ainv = 0:
// z = z0, block Jacobi alone, still a symmetric positive definite preconditioner) and counted (stba_pcg_summary::coarse_failures),
// instead of sending the PCG into NaNs and the LM step into a rejection nobody can explain.
__global__ __launch_bounds__(256) void pg_coarse_finish_kernel(int nc, int np, const double* __restrict__ W, double* __restrict__ Ainv,
                                                               const int* __restrict__ cflag, int* __restrict__ fail_count) {
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    const bool bad = cflag[0] != 0;
    if (idx == 0 && bad) atomicAdd(fail_count, 1);
    if (idx >= (size_t)nc * nc) return;
    const int r = (int)(idx / nc), c = (int)(idx % nc);
    const int hi = max(r, c), lo = min(r, c);
    Ainv[idx] = bad ? 0.0 : -W[((size_t)np + hi) * (2 * (size_t)np) + np + lo];
}

// restriction of a workgroup's 128 nodes: w[node][u] = (P_node^T r_node)[u] sits in LDS; the groups that END in this
// workgroup's range are summed serially in node order (fixed order: same bits everywhere).  Groups of up to 128 nodes lie
// inside one workgroup (128 % agg == 0); larger ones (agg = 256, 512, ...) span agg / 128 workgroups, each of which writes
// its own partial row of rc_part -- the coarse kernel adds the parts in order.
__device__ inline void pg_restrict_store(const double (*wsm)[6], int n, int agg, int node0, double* __restrict__ rc_part) {
    const int t = threadIdx.x;
    if (agg <= PG_NPW) {
        const int ng = PG_NPW / agg;
        if (t < 6 * ng) {
            const int gl = t / 6, u = t % 6;
            const int kb = gl * agg;
            if (node0 + kb < n) {
                double s = 0.0;
                for (int k = 0; k < agg && node0 + kb + k < n; ++k) s += wsm[kb + k][u];
                rc_part[(size_t)((node0 + kb) / agg) * 6 + u] = s;
            }
        }
    } else if (t < 6) {
        double s = 0.0;
        for (int k = 0; k < PG_NPW && node0 + k < n; ++k) s += wsm[k][t];
        rc_part[(size_t)(node0 / PG_NPW) * 6 + t] = s;
    }
}

// PCG start: r = -g, x = 0, z0 = Minv r (into z), restriction of r; partial -> {r.z0, r.r}
__global__ __launch_bounds__(PG_NT) void pg_pcg_init4_kernel(int n, int agg, const double* __restrict__ g, const double* __restrict__ Minv,
                                                            const double* __restrict__ AdP, double* __restrict__ x, double* __restrict__ r,
                                                            double* __restrict__ z, double* __restrict__ rc_part, double* __restrict__ part) {
    __shared__ double wsm[PG_NPW][6];
    const int t = threadIdx.x, nl = t >> 3, k = t & 7;
    const int node0 = blockIdx.x * PG_NPW, node = node0 + nl;
    double a = 0.0, b = 0.0;
    if (node < n && k < 6) {
        double rl[6];
        for (int q = 0; q < 6; ++q) rl[q] = -g[(size_t)node * 6 + q];
        double z0 = 0.0, w = 0.0;
        for (int q = 0; q < 6; ++q) { z0 += Minv[(size_t)node * 36 + k * 6 + q] * rl[q]; if (AdP) w += AdP[(size_t)node * 36 + q * 6 + k] * rl[q]; }
        r[(size_t)node * 6 + k] = rl[k]; x[(size_t)node * 6 + k] = 0.0; z[(size_t)node * 6 + k] = z0;
        wsm[nl][k] = w;
        a = rl[k] * z0; b = rl[k] * rl[k];
    }
    __syncthreads();
    if (AdP) pg_restrict_store(wsm, n, agg, node0, rc_part);
    double out2[2];
    block_sum2_n<PG_NT>(a, b, out2);
    if (t == 0) { part[blockIdx.x * 2] = out2[0]; part[blockIdx.x * 2 + 1] = out2[1]; }
}

// one PCG step on the nodes: q (GATHERED from the edge kernel's u on one rank, read from the all-reduced product with several),
// alpha = rz / p.q, x += alpha p, r -= alpha q, z0 = Minv r, restriction; partial -> {r.z0, r.r}.  Eight lanes per node: lane j takes
// the node's edge ends j, j + 8, ... (all loads of the gather in flight at once -- one lane per node walking its ends was a
// chain of dependent round trips, 19 us for 10 000 nodes in round 3), the six components are summed over the lanes with a
// butterfly, lanes 0..5 then own one component each.
template <bool GATHER>
__global__ __launch_bounds__(PG_NT) void pg_pcg_update4_kernel(int n, int m, int agg, int slot, const PgPcgState* __restrict__ state,
                                                              int nb_a, const double* __restrict__ part_a, int nb_b,
                                                              const double* __restrict__ part_b, const double* __restrict__ Minv,
                                                              const double* __restrict__ AdP, const double* __restrict__ d,
                                                              const int* __restrict__ node_start, const int* __restrict__ end_code,
                                                              const double* __restrict__ u, const double* __restrict__ qin,
                                                              const double* __restrict__ p, double* __restrict__ x, double* __restrict__ r,
                                                              double* __restrict__ z, double* __restrict__ rc_part, double* __restrict__ part_out) {
    __shared__ double wsm[PG_NPW][6];
    __shared__ double s_red[2][PG_NT / 64];
    const int t = threadIdx.x, nl = t >> 3, k = t & 7;
    const int node0 = blockIdx.x * PG_NPW, node = node0 + nl;
    // Everything that does not depend on alpha is REQUESTED first, in one go: the kernel is a chain of memory round trips
    // (~1 us each on a machine this empty), and in program order -- state, partial sums, CSR, edge products, vectors, blocks --
    // it took 14 us for 10 000 nodes.  The `done` flag is looked at only after the requests are out.
    const int done = state->done;
    const double rz = state->rz[slot];
    double pa = 0.0, pb = 0.0;
    for (int q = t; q < nb_a; q += PG_NT) pa += part_a[q * 2];
    if (part_b) for (int q = t; q < nb_b; q += PG_NT) pb += part_b[q * 2];
    double ql[6] = {0, 0, 0, 0, 0, 0};
    double pk = 0.0, rk = 0.0, dk = 0.0, xk = 0.0, mrow[6] = {0, 0, 0, 0, 0, 0}, pcol[6] = {0, 0, 0, 0, 0, 0};
    const bool act = node < n && k < 6;
    const size_t o = (size_t)node * 6 + k;
    if (act) {
        pk = p[o]; rk = r[o]; xk = x[o];
        if (GATHER) dk = d[o]; else dk = qin[o];
        for (int q = 0; q < 6; ++q) mrow[q] = Minv[(size_t)node * 36 + k * 6 + q];
        if (AdP) for (int q = 0; q < 6; ++q) pcol[q] = AdP[(size_t)node * 36 + q * 6 + k];
    }
    if (GATHER && node < n) {
        const int e1 = node_start[node + 1];
        for (int c = node_start[node] + k; c < e1; c += 8) {
            const int code = end_code[c];                              // = 2 e + side: the end's six doubles start at u + 6 code
            const double2* ue = reinterpret_cast<const double2*>(u + (size_t)code * 6);
            const double2 a0 = ue[0], a1 = ue[1], a2 = ue[2];
            ql[0] += a0.x; ql[1] += a0.y; ql[2] += a1.x; ql[3] += a1.y; ql[4] += a2.x; ql[5] += a2.y;
        }
    }
    if (done) return;
    // p.q: one rank: sum |t_e|^2 (edge kernel) + sum d p^2 (direction kernel); several: the dot-product kernel's partials.
    // Fixed order: every workgroup (and every rank) gets the same bits.
    for (int off = 32; off > 0; off >>= 1) { pa += __shfl_down(pa, off, 64); pb += __shfl_down(pb, off, 64); }
    if ((t & 63) == 0) { s_red[0][t >> 6] = pa; s_red[1][t >> 6] = pb; }
    __syncthreads();
    double pq = 0.0, pq2 = 0.0;
    for (int w = 0; w < PG_NT / 64; ++w) { pq += s_red[0][w]; pq2 += s_red[1][w]; }
    pq += pq2;
    const double alpha = (pq > 0.0) ? rz / pq : 0.0;
    if (GATHER) {
        for (int q = 0; q < 6; ++q) {
            ql[q] += __shfl_xor(ql[q], 1, 8);
            ql[q] += __shfl_xor(ql[q], 2, 8);
            ql[q] += __shfl_xor(ql[q], 4, 8);
        }
    }
    if (act) {
        double qk;
        if (GATHER) {
            qk = ql[0];
            if (k == 1) qk = ql[1]; else if (k == 2) qk = ql[2]; else if (k == 3) qk = ql[3]; else if (k == 4) qk = ql[4]; else if (k == 5) qk = ql[5];
            qk += dk * pk;
        } else qk = dk;
        x[o] = xk + alpha * pk;
        rk = rk - alpha * qk;
        r[o] = rk;
    } else rk = 0.0;
    double rl[6];
    for (int q = 0; q < 6; ++q) rl[q] = __shfl(rk, q, 8);
    double a = 0.0, b = 0.0;
    if (act) {
        double z0 = 0.0, w = 0.0;
        for (int q = 0; q < 6; ++q) { z0 += mrow[q] * rl[q]; w += pcol[q] * rl[q]; }
        z[o] = z0;
        wsm[nl][k] = w;
        a = rk * z0; b = rk * rk;
    }
    __syncthreads();
    if (AdP) pg_restrict_store(wsm, n, agg, node0, rc_part);
    double out2[2];
    block_sum2_n<PG_NT>(a, b, out2);
    if (t == 0) { part_out[blockIdx.x * 2] = out2[0]; part_out[blockIdx.x * 2 + 1] = out2[1]; }
}

// coarse correction: zc = Ainv rc (one wave per row; rc = the parts of its group added in order); partial -> rc.zc
__global__ __launch_bounds__(256) void pg_coarse_solve_kernel(int nc, int parts, const PgPcgState* __restrict__ state, const double* __restrict__ Ainv,
                                                              const double* __restrict__ rc_part, double* __restrict__ zc,
                                                              double* __restrict__ part_cz) {
    __shared__ double sw[4];
    const int done = state ? state->done : 0;           // (looked at below, behind the row's first loads)
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int row = blockIdx.x * 4 + w;
    auto rc = [&](int c) {
        const int a = c / 6, u = c % 6;
        double s = 0.0;
        for (int j = 0; j < parts; ++j) s += rc_part[(size_t)(a * parts + j) * 6 + u];
        return s;
    };
    double acc = 0.0;
    if (row < nc)
        for (int c = lane; c < nc; c += 64) acc += Ainv[(size_t)row * nc + c] * rc(c);
    if (done) return;
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_down(acc, o, 64);
    if (lane == 0) {
        double prod = 0.0;
        if (row < nc) { zc[row] = acc; prod = rc(row) * acc; }
        sw[w] = prod;
    }
    __syncthreads();
    if (threadIdx.x == 0) { part_cz[blockIdx.x * 2] = (sw[0] + sw[1]) + (sw[2] + sw[3]); part_cz[blockIdx.x * 2 + 1] = 0.0; }
}

// z = z0 + P zc; rz_new = sum r.z0 + rc.zc; beta = rz_new / rz_old (first: p = z); p = z + beta p; partial -> sum d p^2.
// Workgroup 0 also keeps the books of the solve: rz for the next iteration, the iteration count, and the STOPPING TEST
// |r|^2 <= eta^2 |b|^2 (or the iteration cap) -- once `done` is set every later kernel of the solve returns at once, so the
// host can enqueue iterations ahead of what it knows (it polls the exported block in mapped memory).
__global__ __launch_bounds__(PG_NT) void pg_pcg_dir4_kernel(int n, int agg, int slot, int first, double eta, int max_iters, PgPcgState* __restrict__ state,
                                                           double* __restrict__ exp_, int nb_rz, const double* __restrict__ part_rz, int nb_cz,
                                                           const double* __restrict__ part_cz, const double* __restrict__ AdP,
                                                           const double* __restrict__ zc, const double* __restrict__ z, const double* __restrict__ d,
                                                           double* __restrict__ p, double* __restrict__ part_dp) {
    __shared__ double s_red[3][PG_NT / 64];
    const int t = threadIdx.x;
    // (as in the update kernel: every load that does not depend on beta is requested before anything is waited for)
    const int was_done = first ? 0 : state->done;
    const double rzo = first ? 1.0 : state->rz[slot];
    double s0 = 0.0, s1 = 0.0, s2 = 0.0;
    for (int q = t; q < nb_rz; q += PG_NT) { s0 += part_rz[q * 2]; s2 += part_rz[q * 2 + 1]; }
    if (part_cz) for (int q = t; q < nb_cz; q += PG_NT) s1 += part_cz[q * 2];
    const int nl = t >> 3, k = t & 7;
    const int node = blockIdx.x * PG_NPW + nl;
    const bool act = node < n && k < 6;
    const size_t o = (size_t)node * 6 + k;
    double zk = 0.0, pold = 0.0, dk = 0.0;
    if (act) {
        zk = z[o]; dk = d[o];
        if (!first) pold = p[o];
        if (AdP) {
            const int a = node / agg;
            for (int q = 0; q < 6; ++q) zk += AdP[(size_t)node * 36 + k * 6 + q] * zc[(size_t)a * 6 + q];
        }
    }
    if (was_done) {
        if (blockIdx.x == 0 && t == 0) {
            const int tk = state->ticks + 1;
            state->ticks = tk;
            if (exp_) {        // (the same block again under the new tick)
                const double px[PX_COUNT] = {state->rr0, state->rr, (double)state->iters, (double)state->done, (double)state->hit_cap};
                stamped_store_thread(exp_, px, PX_COUNT, (double)tk);
            }
        }
        return;
    }
    for (int off = 32; off > 0; off >>= 1) { s0 += __shfl_down(s0, off, 64); s1 += __shfl_down(s1, off, 64); s2 += __shfl_down(s2, off, 64); }
    if ((t & 63) == 0) { s_red[0][t >> 6] = s0; s_red[1][t >> 6] = s1; s_red[2][t >> 6] = s2; }
    __syncthreads();
    double rzn = 0.0, rcz = 0.0, rr = 0.0;
    for (int w = 0; w < PG_NT / 64; ++w) { rzn += s_red[0][w]; rcz += s_red[1][w]; rr += s_red[2][w]; }
    rzn += rcz;
    const double beta = first ? 0.0 : ((rzo > 0.0) ? rzn / rzo : 0.0);
    double dp2 = 0.0;
    if (act) {
        const double pv = first ? zk : zk + beta * pold;
        p[o] = pv;
        dp2 = dk * pv * pv;
    }
    double out2[2];
    block_sum2_n<PG_NT>(dp2, 0.0, out2);
    if (t == 0) { part_dp[blockIdx.x * 2] = out2[0]; part_dp[blockIdx.x * 2 + 1] = 0.0; }
    if (blockIdx.x == 0 && t == 0) {
        int iters, done, cap = 0, tk;
        double rr0, tol2;
        if (first) {
            rr0 = rr; tol2 = eta * eta * rr0; iters = 0; tk = 1;
            done = !(rr0 > 0.0) || !isfinite(rr0) || !isfinite(rzn);
        } else {
            rr0 = state->rr0; tol2 = state->tol2; iters = state->iters + 1; tk = state->ticks + 1;
            done = !(rr > tol2);                              // (also ends the solve on a NaN)
            if (!done && iters >= max_iters) { done = 1; cap = 1; }
        }
        state->rz[slot ^ 1] = rzn;
        state->rr0 = rr0; state->tol2 = tol2; state->rr = rr; state->iters = iters; state->done = done; state->hit_cap = cap; state->ticks = tk;
        if (exp_) {
            const double px[PX_COUNT] = {rr0, rr, (double)iters, (double)done, (double)cap};
            stamped_store_thread(exp_, px, PX_COUNT, (double)tk);
        }
    }
}

// ================================================================= round 5: the PCG solve of an LM iteration as ONE kernel
// Four launches per PCG iteration cost ~44 us for ~34 us of kernels (C4), every kernel a chain of three memory round trips on an
// empty machine.  Round 3's persistent loop (four grid BARRIERS per iteration, 59 us) was slower still; what a barrier costs is not
// the exchange but the counter: arrive, wait for the count, then fetch the data.  Here nothing is counted.  One workgroup per
// GROUP of the coarse space (<= 64 nodes, <= 256 groups: all resident, one per CU) keeps its nodes' x, r, p, s, u, w and its six rows
// of the coarse inverse in REGISTERS for the whole solve, and an iteration has two exchanges, each a block of data with a STAMP
// behind it (agent-scope write-through stores, agent-scope loads: no fence, no cache invalidate):
//   A  the group's slice of u = M^-1 r; an edge end waits for the stamp of the ONE group that owns its remote node, reads 48 bytes;
//   B  nine doubles per group -- the partial sums of (r, u), (w, u), (r, r) and the group's six entries of P^T w -- which every
//      group reads from every group: an all-gather of 157 x 72 bytes at C4.
// Two exchanges suffice because the iteration is the Chronopoulos-Gear form of PCG (w = A u instead of q = A p; p and s = A p by
// recurrence; both dot products of a step in ONE reduction), and because the coarse residual is carried by recurrence, replicated
// in every group: r_c <- r_c - alpha P^T s, P^T s = P^T w + beta P^T s -- so the restriction never needs a gather of its own.
// Measured skeleton (tools/exp/pcg_skeleton.hip, no arithmetic): 6.0 us per iteration (A 2.6, B 3.8).
// The matrix is applied ASSEMBLED: (H_ii + D_i) u_i from the diagonal blocks the linearisation leaves, plus one 6 x 6 block
// B_e = Ji^T Jj per edge END (its transpose for the other end), written once per linearisation in the order the groups read
// them (pg_offdiag_kernel), 36 coalesced loads per end and iteration out of the XCD's L2.
// Several ranks (edge shards) keep the launch-per-kernel path: their product needs a cross-rank sum in every iteration.
// (PP_T, PP_VCAP, PP_NCMAX, PP_SLOT, PP_STAMP and pp_lds_bytes, the layout the host sizes and this kernel indexes: pg_plan.hpp)
constexpr int PP_TIMED_OUT = 2;      // PgPcgState::hit_cap: a stamp never came (the workgroups were not all resident): the caller repeats the solve with launches

struct PpArgs {
    int n, agg, log2agg, na, nc, base, max_iters;
    double eta;
    const int *node_start, *end_rem;
    const double *Bend, *Hd, *d, *Minv, *AdP, *Ainv, *g;
    double *x, *ubuf, *pbuf;
    int *ustamp, *pstamp;
    PgPcgState* state;
    long long spin_limit; // how long a workgroup waits for a stamp, in ticks of wall_clock64 (100 MHz); 0: not at all (the test of the way back)
    double eta_c;         // tolerance on |P^T r| / |P^T r_0| in the stopping test (<= 0: none)
    int fences;           // 1: the stamps are published behind a RELEASE fence and read in front of an ACQUIRE fence (agent scope); 0: compiler barriers only
    long long* tdbg;      // debug builds: time per phase (group 0), else null
};

__device__ __forceinline__ int pp_ld_i(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ double pp_ld(const double* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void pp_st(double* p, double v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
// THE MEMORY ORDER OF THE TWO EXCHANGES (advisor, round 5).  Producer: data with agent-scope stores (write-through), s_waitcnt
// vmcnt(0) -- every store acknowledged --, workgroup barrier, then the stamp.  Consumer: polls the stamp, then loads the data with
// agent-scope loads (never from the L1).  What the hardware orders by itself (a load is ISSUED after the poll's branch has seen the
// stamp; stores are acknowledged before the stamp is issued) the COMPILER must not undo: both sides carry a compiler barrier.
// With PpArgs::fences the stamp is also stored behind an agent-scope release fence and the data loaded behind an acquire fence --
// the formally complete protocol; measured against the barrier-only form in tools/dbg/c4_async.py (round 6).
__device__ __forceinline__ void pp_publish(int* stamp, int value, int fences) {
    if (fences) __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    else asm volatile("" ::: "memory");
    __hip_atomic_store(stamp, value, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// waits until *stamp >= want; the limit is WALL-CLOCK time (a slow but live peer must not send the engine to the launch path for
// good: until round 5 the limit was a count of polls), looked at every 32 polls
__device__ __forceinline__ bool pp_await(const int* stamp, int want, long long limit_ticks, int fences) {
    bool ok = true;
    if (pp_ld_i(stamp) - want < 0) {
        const long long t0 = wall_clock64();
        unsigned spins = 0;
        while (pp_ld_i(stamp) - want < 0) {
            __builtin_amdgcn_s_sleep(1);
            if (limit_ticks <= 0 || ((++spins & 31u) == 0 && wall_clock64() - t0 > limit_ticks)) { ok = false; break; }
        }
    }
    if (fences) __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    else asm volatile("" ::: "memory");
    return ok;
}

// B_e = Ji^T Jj of every edge, stored COMPONENT-major over the CSR positions of the edge ENDS ([36][2 m]): column end_pos[2 e] (the
// end at i, which multiplies u_j) gets B_e, column end_pos[2 e + 1] (the end at j, which multiplies u_i) its transpose
__global__ __launch_bounds__(256) void pg_offdiag_kernel(int m, const double* __restrict__ Ji, const double* __restrict__ Jj,
                                                         const int* __restrict__ end_pos, double* __restrict__ Bend) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= m) return;
    double A[36], B[36];
    for (int k = 0; k < 36; ++k) { A[k] = Ji[(size_t)k * m + e]; B[k] = Jj[(size_t)k * m + e]; }
    const size_t m2 = 2 * (size_t)m;
    const size_t c0 = (size_t)end_pos[2 * e], c1 = (size_t)end_pos[2 * e + 1];
    for (int a = 0; a < 6; ++a)
        for (int b = 0; b < 6; ++b) {
            double s = 0.0;
            for (int r = 0; r < 6; ++r) s += A[r * 6 + a] * B[r * 6 + b];
            Bend[(size_t)(a * 6 + b) * m2 + c0] = s;
            Bend[(size_t)(b * 6 + a) * m2 + c1] = s;
        }
}

#ifdef STBA_DEBUG_KNOBS
#define PP_STAMP_T(i) do { if (a.tdbg && grp == 0 && t == 0) { const long long now_ = wall_clock64(); a.tdbg[i] += now_ - tlast; tlast = now_; } } while (0)
#else
#define PP_STAMP_T(i) do { } while (0)
#endif
__global__ __launch_bounds__(PP_T) void pg_pcg_persistent_kernel(PpArgs a) {
    extern __shared__ double pp_sm[];
    __shared__ int s_abort;
    const int t = threadIdx.x, grp = blockIdx.x;
    const int n = a.n, agg = a.agg, na = a.na, nc = a.nc;
    double* rc = pp_sm;                       // [nc]   coarse residual P^T r, replicated in every group
    double* pts = rc + nc;                    // [nc]   P^T s
    double* gat = pts + nc;                   // [na][PP_SLOT]  the gathered block of exchange B
    double* ul = gat + (size_t)na * PP_SLOT;  // [384]  this group's u (the diagonal term reads it)
    double* rl = ul + 384;                    // [384]  this group's r (block Jacobi reads a node's six)
    double* vbuf = rl + 384;                  // [PP_VCAP][6]  products of the edge ends
    double* red = vbuf + (size_t)PP_VCAP * 6; // [128] scratch of the gathered sums
    double* sc = red + 128;                   // [16]  the group's sums | zc at 8..13
    if (t == 0) s_abort = 0;
    // ---- what a thread keeps for the whole solve
    const int nl = t / 6, q = t - nl * 6;
    const int node = grp * agg + nl;
    const bool act = t < agg * 6 && node < n;
    const size_t o = (size_t)node * 6 + q;
    double mrow[6] = {0, 0, 0, 0, 0, 0}, hrow[6] = {0, 0, 0, 0, 0, 0}, prow[6] = {0, 0, 0, 0, 0, 0};
    double r = 0.0, x = 0.0, p = 0.0, s = 0.0, u = 0.0, w = 0.0;
    int e0 = 0, e1 = 0;
    const int c0 = a.node_start[min(n, grp * agg)], c1 = a.node_start[min(n, (grp + 1) * agg)];
    if (act) {
        for (int b = 0; b < 6; ++b) {
            mrow[b] = a.Minv[(size_t)node * 36 + q * 6 + b];
            hrow[b] = a.Hd[(size_t)node * 36 + q * 6 + b];
            prow[b] = a.AdP[(size_t)node * 36 + q * 6 + b];
        }
        hrow[q] += a.d[o];
        r = -a.g[o];
        e0 = a.node_start[node] - c0; e1 = a.node_start[node + 1] - c0;
    }
    double acol[3][6];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const int c = t + j * PP_T;
#pragma unroll
        for (int rr_ = 0; rr_ < 6; ++rr_) acol[j][rr_] = (c < nc) ? a.Ainv[(size_t)(grp * 6 + rr_) * nc + c] : 0.0;
    }
    const size_t m2 = (size_t)a.node_start[n];        // edge ends = 2 m
    const int rem0 = (c0 + t < c1) ? a.end_rem[c0 + t] : 0;
    __syncthreads();

    // K values per thread -> the group's sums in sc[off .. off + K).  Through LDS in three fixed steps (512 -> 32 -> 1 per value): a
    // shuffle tree is a chain of ds_bpermute round trips, 6 per value -- 54 of them for the nine sums took 2 us of a 15 us iteration.
    // The buffer is the edge ends' product buffer, which is spent whenever sums are made.
    auto group_sum = [&](const double* v, int K, int off) {
        double* tr = vbuf;                       // [K][PP_T]
        double* p2 = vbuf + 9 * PP_T;            // [K][33]
        __syncthreads();                         // (the last reader of the products is through)
        for (int k = 0; k < K; ++k) tr[k * PP_T + t] = v[k];
        __syncthreads();
        if (t < K * 32) {
            const int k = t >> 5, j = t & 31;
            double y = 0.0;
#pragma unroll
            for (int i = 0; i < PP_T / 32; ++i) y += tr[k * PP_T + j + 32 * i];
            p2[k * 33 + j] = y;
        }
        __syncthreads();
        if (t < K) {
            double y = 0.0;
#pragma unroll
            for (int j = 0; j < 32; ++j) y += p2[t * 33 + j];
            sc[off + t] = y;
        }
        __syncthreads();
    };
    // exchange B: sc[0 .. K) of every group -> gat[group][0 .. K)
    auto all_gather = [&](int round, int K) {
        double* mine = a.pbuf + ((size_t)(round & 1) * na + grp) * PP_SLOT;
        if (t < K) { pp_st(mine + t, sc[t]); asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }
        __syncthreads();
        if (t == 0) pp_publish(&a.pstamp[grp * PP_STAMP], a.base + round + 1, a.fences);
        if (t < na) {
            const bool ok = pp_await(&a.pstamp[t * PP_STAMP], a.base + round + 1, a.spin_limit, a.fences);
            if (!ok) s_abort = 1;
            if (ok) {
                const double* src = a.pbuf + ((size_t)(round & 1) * na + t) * PP_SLOT;
                for (int k = 0; k < K; ++k) gat[t * PP_SLOT + k] = pp_ld(src + k);
            }
        }
        __syncthreads();
    };
    // the first K entries of the gathered block summed over the groups (the same order in every group: every group gets the same bits)
    auto gathered_sums = [&](int K) {
        double* p2 = red;                        // [K][33]
        if (t < K * 32) {
            const int k = t >> 5, j = t & 31;
            double y = 0.0;
            for (int i = j; i < na; i += 32) y += gat[i * PP_SLOT + k];
            p2[k * 33 + j] = y;
        }
        __syncthreads();
        if (t < K) {
            double y = 0.0;
#pragma unroll
            for (int j = 0; j < 32; ++j) y += p2[t * 33 + j];
            sc[t] = y;
        }
        __syncthreads();
    };
    double rc2 = 0.0;                  // |P^T r|^2 of the current residual (the same bits in every group)
    auto coarse_and_u = [&]() {        // zc = (own six rows of the inverse) rc; u = Minv r + P zc
        double zp[7];
#pragma unroll
        for (int rr_ = 0; rr_ < 6; ++rr_) {
            double y = 0.0;
#pragma unroll
            for (int j = 0; j < 3; ++j) { const int c = t + j * PP_T; if (c < nc) y += acol[j][rr_] * rc[c]; }
            zp[rr_] = y;
        }
        {
            double y = 0.0;
#pragma unroll
            for (int j = 0; j < 3; ++j) { const int c = t + j * PP_T; if (c < nc) y += rc[c] * rc[c]; }
            zp[6] = y;
        }
        if (t < 384) rl[t] = r;
        group_sum(zp, 7, 8);
        rc2 = sc[14];
        double z0 = 0.0;
        if (act) {
            for (int b = 0; b < 6; ++b) z0 += mrow[b] * rl[nl * 6 + b];
            for (int b = 0; b < 6; ++b) z0 += prow[b] * sc[8 + b];
        }
        u = z0;
    };
    auto finish = [&](int iters, int cap, double rr0, double rr, double tol2) {
        if (act) a.x[o] = x;
        if (grp == 0 && t == 0) {
            a.state->rr0 = rr0; a.state->rr = rr; a.state->tol2 = tol2; a.state->iters = iters; a.state->done = 1; a.state->hit_cap = cap;
        }
    };

    // ---- start: x = 0, r = -g; |r|^2 and P^T r gathered; u = M^-1 r
    {
        double v[7];
        v[0] = r * r;
        for (int b = 0; b < 6; ++b) v[1 + b] = prow[b] * r;
        group_sum(v, 7, 0);
        all_gather(0, 7);
        if (s_abort) { finish(0, PP_TIMED_OUT, 0.0, 0.0, 0.0); return; }
        for (int c = t; c < nc; c += PP_T) { rc[c] = gat[(c / 6) * PP_SLOT + 1 + (c % 6)]; pts[c] = 0.0; }
        gathered_sums(1);
    }
    const double rr0 = sc[0];
    __syncthreads();
    if (!(rr0 > 0.0) || !isfinite(rr0)) { finish(0, 0, rr0, rr0, 0.0); return; }
    const double tol2 = a.eta * a.eta * rr0;
    coarse_and_u();
    // (round 6) the COARSE residual has a tolerance of its own: the coarse space holds the smooth, weakly constrained modes of the
    // graph, where a residual of eta |g| is a large error -- with the inverse of the PREVIOUS operator as coarse solver (coarse_async)
    // that error is what moves the LM trajectory away from the exact-step one.  eta_c <= 0: no such test
    const double tolc2 = a.eta_c > 0.0 ? a.eta_c * a.eta_c * rc2 : -1.0;
    double gamma_old = 1.0, alpha_old = 1.0;
    const size_t N6 = (size_t)n * 6;
    long long tlast = wall_clock64();
    (void)tlast;
    for (int k = 0;; ++k) {
        PP_STAMP_T(6);
        // ---- exchange A: publish the group's u
        double* ub = a.ubuf + (size_t)(k & 1) * N6;
        if (act) { pp_st(ub + o, u); asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }
        if (t < 384) ul[t] = u;
        __syncthreads();
        if (t == 0) pp_publish(&a.ustamp[grp * PP_STAMP], a.base + k + 1, a.fences);
        PP_STAMP_T(0);
        // ---- off-diagonal blocks times the remote ends' u
        for (int c = c0 + t, pass = 0; c < c1; c += PP_T, ++pass) {
            double B[36];
#pragma unroll
            for (int b = 0; b < 36; ++b) B[b] = a.Bend[(size_t)b * m2 + c];
            // (the first pass's remote node is kept: one round trip less in front of the poll.  Half the groups have more than 512 ends
            // at C4 and make a second trip; measured and not kept: both trips' stamps polled together and the block loads behind the
            // poll, 1070 against 1090 LM it/s -- the loads no longer overlap the wait; both ends' blocks in flight at once: 184-472
            // bytes of scratch per lane, 780 LM it/s)
            const int rem = pass == 0 ? rem0 : a.end_rem[c];
            const int* stamp = &a.ustamp[(rem >> a.log2agg) * PP_STAMP];
            const bool ok = pp_await(stamp, a.base + k + 1, a.spin_limit, a.fences);
            if (!ok) s_abort = 1;
            double ur[6] = {0, 0, 0, 0, 0, 0};
            if (ok) for (int b = 0; b < 6; ++b) ur[b] = pp_ld(ub + (size_t)rem * 6 + b);
#pragma unroll
            for (int aa = 0; aa < 6; ++aa) {
                double y = 0.0;
#pragma unroll
                for (int b = 0; b < 6; ++b) y += B[aa * 6 + b] * ur[b];
                vbuf[(size_t)(c - c0) * 6 + aa] = y;
            }
        }
        __syncthreads();
        if (s_abort) { finish(k, PP_TIMED_OUT, rr0, 0.0, tol2); return; }
        PP_STAMP_T(1);
        w = 0.0;
        if (act) {
            for (int b = 0; b < 6; ++b) w += hrow[b] * ul[nl * 6 + b];
            for (int e = e0; e < e1; ++e) w += vbuf[(size_t)e * 6 + q];
        }
        // ---- exchange B: (r, u), (w, u), (r, r), P^T w
        {
            double v[9];
            v[0] = r * u; v[1] = w * u; v[2] = r * r;
            for (int b = 0; b < 6; ++b) v[3 + b] = prow[b] * w;
            group_sum(v, 9, 0);
            PP_STAMP_T(2);
            all_gather(k + 1, 9);
            PP_STAMP_T(3);
            if (s_abort) { finish(k, PP_TIMED_OUT, rr0, 0.0, tol2); return; }
            gathered_sums(3);
        }
        const double gamma = sc[0], delta = sc[1], rr = sc[2];
        // the residual of k updates: the stopping test (the first iteration always runs, as with the launches)
        if (k > 0 && !(rr > tol2) && !(tolc2 >= 0.0 && rc2 > tolc2)) { finish(k, 0, rr0, rr, tol2); return; }
        if (k >= a.max_iters) { finish(k, 1, rr0, rr, tol2); return; }
        const double beta = (k == 0) ? 0.0 : gamma / gamma_old;
        const double den = (k == 0) ? delta : delta - beta * gamma / alpha_old;
        if (!(den > 0.0) || !isfinite(den) || !isfinite(gamma)) { finish(k, 1, rr0, rr, tol2); return; }     // (breakdown: never seen; reported as a capped solve)
        const double alpha = gamma / den;
        p = u + beta * p; s = w + beta * s;
        x += alpha * p; r -= alpha * s;
        for (int c = t; c < nc; c += PP_T) {
            const double ps = gat[(c / 6) * PP_SLOT + 3 + (c % 6)] + beta * pts[c];
            pts[c] = ps;
            rc[c] -= alpha * ps;
        }
        gamma_old = gamma; alpha_old = alpha;
        __syncthreads();
        PP_STAMP_T(4);
        coarse_and_u();
        PP_STAMP_T(5);
    }
}

// trial point of an LM iteration: the scalars the host decides on, summed on the device and written to mapped host memory
// (one rank) or to a device block the cross-rank sum goes over first.  out: {cost2_new, |J x|^2, g.x, |dx|^2, |x|^2, seq}
__global__ __launch_bounds__(256) void pg_trial_finish_kernel(int nb_e, const double* __restrict__ part_e, int nb_tt,
                                                              const double* __restrict__ part_tt, int nb_u, const double* __restrict__ part_u,
                                                              const PgPcgState* __restrict__ state, double* __restrict__ out, double seq) {
    const double c2 = sum_partials_dev(part_e, nb_e, 1, 0);
    const double tt = sum_partials_dev(part_tt, nb_tt, 2, 0);
    const double gx = sum_partials_dev(part_u, nb_u, 4, 0);
    const double s2 = sum_partials_dev(part_u, nb_u, 4, 1);
    const double x2 = sum_partials_dev(part_u, nb_u, 4, 2);
    __shared__ double hp[8];
    if (threadIdx.x == 0) {
        hp[0] = c2; hp[1] = tt; hp[2] = gx; hp[3] = s2; hp[4] = x2;
        hp[5] = state ? (double)state->iters : 0.0; hp[6] = state ? (double)state->hit_cap : 0.0; hp[7] = state ? state->rr0 : 0.0;
    }
    __syncthreads();
    if (threadIdx.x < 64) stamped_store_wave(out, hp, 8, seq, threadIdx.x);       // (a stamped block: common.hpp)
}
// linearisation: {cost2, |g|_inf, seq}
__global__ __launch_bounds__(256) void pg_linear_finish_kernel(int nb_e, const double* __restrict__ part_e, int nb_g, const double* __restrict__ part_g,
                                                               double* __restrict__ out, double seq) {
    const double c2 = sum_partials_dev(part_e, nb_e, 1, 0);
    const double g2 = sum_partials_dev(part_g, nb_g, 2, 0);
    __shared__ double sq[256];
    double mx = 0.0;
    for (int k = threadIdx.x; k < nb_g; k += 256) mx = fmax(mx, part_g[2 * k + 1]);
    sq[threadIdx.x] = mx;
    __syncthreads();
    __shared__ double hp[3];
    if (threadIdx.x == 0) {
        for (int k = 1; k < 256; ++k) mx = fmax(mx, sq[k]);
        hp[0] = c2; hp[1] = mx; hp[2] = g2;
    }
    __syncthreads();
    if (threadIdx.x < 64) stamped_store_wave(out, hp, 3, seq, threadIdx.x);
}
__global__ void pg_export_kernel(int cnt, const double* __restrict__ src, double* __restrict__ out, double seq) {
    stamped_store_wave(out, src, cnt, seq, threadIdx.x);      // (one wave; src is device memory the previous kernel or collective left)
}

// trial poses + statistics of the step: partial[b] = {g.x, |x_new - x|^2, |x|^2, 0}
__global__ __launch_bounds__(256) void pg_update4_kernel(int n_nodes, const double* __restrict__ poses, const double* __restrict__ dx,
                                                         const double* __restrict__ g, const unsigned char* __restrict__ fixed,
                                                         double* __restrict__ poses_new, double* __restrict__ partial) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    double a = 0.0, b = 0.0, c = 0.0;
    if (i < n_nodes) {
        double T[7], d[6], Tn[7];
        for (int k = 0; k < 7; ++k) T[k] = poses[(size_t)i * 7 + k];
        const bool fx = fixed && fixed[i];
        for (int k = 0; k < 6; ++k) { d[k] = fx ? 0.0 : dx[(size_t)i * 6 + k]; c += g[(size_t)i * 6 + k] * d[k]; }
        if (fx) for (int k = 0; k < 7; ++k) Tn[k] = T[k];
        else se3_retract(T, d, Tn);
        for (int k = 0; k < 7; ++k) {
            poses_new[(size_t)i * 7 + k] = Tn[k];
            if (!fx) { a += (Tn[k] - T[k]) * (Tn[k] - T[k]); b += T[k] * T[k]; }
        }
    }
    double out2[2], out3[2];
    block_sum2(a, b, out2);
    __syncthreads();
    block_sum2(c, 0.0, out3);
    if (threadIdx.x == 0) { partial[blockIdx.x * 4] = out3[0]; partial[blockIdx.x * 4 + 1] = out2[0]; partial[blockIdx.x * 4 + 2] = out2[1]; partial[blockIdx.x * 4 + 3] = 0.0; }
}

}  // namespace
}  // namespace stba

using namespace stba;

struct stba_pg {
    int n = 0, m = 0;
    hipStream_t st = nullptr;
    bool own = false;
    DevBuf<double> poses[2];
    int cur = 0;
    DevBuf<int> ei, ej;
    DevBuf<double> meas, r, Ji, Jj, g, Minv, d, scale, x, rr, z, p, q, part_e, part_a, part_b, part_c, part_d;
    double* Hd = nullptr;               // (inside g)
    DevBuf<unsigned char> fixed;
    int nb_nodes = 1, nb_vec = 1, nb_edges = 1;
    // one rank: the edge ends (edge * 2 + side) of every node as a CSR, and the per-edge products u = (Ji^T t | Jj^T t) [12][m]
    DevBuf<int> node_start, end_code;
    DevBuf<double> u;
    // multi-GPU: this engine holds one shard of the EDGES, all nodes are replicated; the hook sums the
    // gradient | diagonal blocks, every matrix-vector product and the cost across ranks
    stba_allreduce_fn ar = nullptr;
    void* ar_user = nullptr;
    int rank = 0, world = 1;
    DevBuf<double> scalar;              // one device double for the cost sums
    // ---- round 4: coarse space of the two-level preconditioner (see the header) and the device-side PCG control
    PgCoarsePlan coarse;                                 // its sizes (pg_plan.hpp); agg 0: none planned yet, -1: off
    DevBuf<int> end_node;                                // owner node of every edge end of the CSR
    DevBuf<double> AdP, Ac0, W, Ainv, inv_work, rc_part, zc, part_cz, part_u, scal_dev, contrib, Dc;
    DevBuf<int> cflag;               // [0]: pivot flag of the coarse factorisation, [1]: coarse operators that failed (this solve)
    DevBuf<PgPcgState> state;
    MappedBuffer exp;                                    // the launch-path PCG's stamped block (PX_*)
    double fin_vals[8] = {0};                            // the host's validated copy of the last trial / linearisation block
    MappedBuffer fin;                                    // the trial / linearisation scalars' stamped block
    double seq = 0.0;
    int nb_nodes4 = 1;
    // ---- round 5: the PCG solve as one persistent kernel (pg_pcg_persistent_kernel)
    DevBuf<int> end_pos, end_rem;                        // CSR position of the edge end 2 e + side | remote node of the end at a CSR position
    DevBuf<double> Bend, ubuf, pbuf;
    DevBuf<int> ustamp, pstamp;
    int pp_base = 0;                                     // stamps only grow: the next solve starts behind the last one's
    bool bend_valid = false, pp_disabled = false;
    std::vector<int> node_start_host;                    // what the engine keeps of its PgEnds: node_start, for pg_plan_coarse
    bool coarse_valid = false;
    double coarse_radius = 0.0;
    // ---- round 6: the coarse inverse OFF the critical path (stba_pcg_options::coarse_async): a second stream inverts the coarse
    // operator of LM iteration k while the first runs iteration k's PCG with the inverse made during iteration k - 1
    hipStream_t st2 = nullptr;
    hipEvent_t ev_in = nullptr, ev_read = nullptr, ev_job[2] = {nullptr, nullptr};
    DevBuf<double> Ainv2;            // the second buffer of the pair (Ainv is the first)
    hipEvent_t ev_t[2] = {nullptr, nullptr};      // stba_lm_options::phase_timing: around the linear solve
    bool job_in_flight = false, job_reads_pending = false, ac0_valid = false;
    stba_pcg_summary last_pcg;
    // host copies of the graph for stba_pg_covariance's gauge check (pg_covariance.hip), which runs before any device work
    std::vector<int> h_ei, h_ej;
    std::vector<unsigned char> h_fixed;
    // per-edge square-root information W_e, component-major [36][m] like Ji (stba_pg_set_information / _sqrt_information); NULL: every
    // edge weighted by the identity, and pg_linearize launches the kernel without the whitening
    DevBuf<double> Winfo;
    // per-edge robust losses (stba_pg_set_loss): kind (STBA_LOSS_*), a, b, scale, each [m]; all NULL: no edge has a loss, and
    // pg_linearize launches a kernel without the corrector
    DevBuf<int> loss_kind;
    DevBuf<double> loss_a, loss_b, loss_scale;
};

namespace stba {
namespace {
// Everything of an engine that is not memory, then the engine: its DevBuf members free themselves in `delete`.  Both streams are
// synchronised FIRST (nothing on the device reads a buffer that is about to go); then the Cholesky's per-stream cache forgets the
// second one, then the events, the mapped blocks and the streams, and the buffers last.
void pg_free(stba_pg* g) {
    if (g->st) (void)hipStreamSynchronize(g->st);
    if (g->st2) { (void)hipStreamSynchronize(g->st2); chol_forget_stream(g->st2); (void)hipStreamDestroy(g->st2); }
    if (g->ev_in) (void)hipEventDestroy(g->ev_in);
    if (g->ev_read) (void)hipEventDestroy(g->ev_read);
    for (auto& e : g->ev_job) if (e) (void)hipEventDestroy(e);
    for (auto& e : g->ev_t) if (e) (void)hipEventDestroy(e);
    g->exp.release();
    g->fin.release();
    if (g->own && g->st) (void)hipStreamDestroy(g->st);
    delete g;
}

double host_sum(hipStream_t st, const double* dev, int n, int stride, int off, std::vector<double>& buf) {
    buf.resize((size_t)n * stride);
    (void)hipMemcpyAsync(buf.data(), dev, buf.size() * sizeof(double), hipMemcpyDeviceToHost, st);
    (void)hipStreamSynchronize(st);
    double s = 0.0;
    for (int k = 0; k < n; ++k) s += buf[(size_t)k * stride + off];
    return s;
}

int pg_linearize(stba_pg* g, int which, bool jac) {
    // (an engine that holds square-root information runs a whitening instantiation, one that holds a loss table a robust one, every
    // other one the kernel without either)
    auto launch = [&](auto kernel) {
        hipLaunchKernelGGL(kernel, dim3(g->nb_edges), dim3(256), 0, g->st, g->m, g->poses[which], g->ei, g->ej,
                           g->meas, g->fixed, jac ? 1 : 0, jac ? g->r : nullptr, g->Ji, g->Jj, g->part_e, jac ? g->contrib : nullptr,
                           (const double*)g->Winfo, (const int*)g->loss_kind, (const double*)g->loss_a, (const double*)g->loss_b,
                           (const double*)g->loss_scale);
    };
    if (g->loss_kind) { if (g->Winfo) launch(pg_linearize_kernel<true, true>); else launch(pg_linearize_kernel<false, true>); }
    else if (g->Winfo) launch(pg_linearize_kernel<true, false>);
    else launch(pg_linearize_kernel<false, false>);
    STBA_HIP(hipGetLastError());
    if (jac) g->bend_valid = false;
    return STBA_OK;
}

// the all-reduce hook over `count` doubles at `buf`, on the engine's stream (one rank: nothing)
int pg_hook(stba_pg* g, double* buf, size_t count) {
    if (g->ar && g->ar(g->ar_user, buf, count, g->st) != 0) return fail(STBA_ERR_CALLBACK, "all-reduce hook failed");
    return STBA_OK;
}

// gradient | diagonal blocks of the last pg_linearize(jac), gathered per node
void pg_gather_blocks(stba_pg* g) {
    hipLaunchKernelGGL(pg_gather_blocks_kernel, dim3(g->nb_nodes4), dim3(PG_NT), 0, g->st, g->n, g->node_start, g->end_code, g->contrib, g->g, g->Hd);
}

// q = (J^T J [+ D]) v.  Sharded: every rank applies its edges, rank 0 alone adds the diagonal term, and the
// hook sums the 6n-vector (the only data-path collective of a PCG iteration: every other vector operation
// is replicated and bit-identical on all ranks).
int pg_apply(stba_pg* g, const double* v, double* q, bool with_d) {
    hipLaunchKernelGGL(pg_diag_mul_kernel, dim3(g->nb_vec), dim3(256), 0, g->st, 6 * g->n, g->d, v, q,
                       (with_d && g->rank == 0) ? 1 : 0);
    hipLaunchKernelGGL(pg_matvec_kernel, dim3(g->nb_edges), dim3(256), 0, g->st, g->m, g->ei, g->ej, g->Ji, g->Jj, v, q);
    STBA_HIP(hipGetLastError());
    return pg_hook(g, q, (size_t)6 * g->n);
}

// sum of a host scalar across ranks (through one device double and the hook)
int pg_sum_ranks(stba_pg* g, double* v) {
    if (!g->ar) return STBA_OK;
    STBA_HIP(hipMemcpyAsync(g->scalar, v, sizeof(double), hipMemcpyHostToDevice, g->st));
    STBA_TRY(pg_hook(g, g->scalar, 1));
    STBA_HIP(hipMemcpyAsync(v, g->scalar, sizeof(double), hipMemcpyDeviceToHost, g->st));
    STBA_HIP(hipStreamSynchronize(g->st));
    return STBA_OK;
}
}  // namespace

// ---- what pg_covariance.hip sees of the engine (pg_covariance.hpp)
void pg_cov_graph(const stba_pg* g, PgCovGraph* out) {
    out->n = g->n; out->m = g->m;
    out->ei = g->h_ei.data(); out->ej = g->h_ej.data();
    out->fixed = g->h_fixed.empty() ? nullptr : g->h_fixed.data();
    out->several_ranks = g->ar != nullptr || g->world > 1;
}
int pg_cov_linearize(stba_pg* g, PgCovDevice* out) {
    // (a coarse inverse of the last solve may still be reading the diagonal blocks on the second stream)
    if (g->st2 && g->job_in_flight) STBA_HIP(hipStreamSynchronize(g->st2));
    STBA_TRY(pg_linearize(g, g->cur, true));
    pg_gather_blocks(g);
    STBA_HIP(hipGetLastError());
    out->st = g->st; out->node_start = g->node_start; out->end_code = g->end_code; out->end_rem = g->end_rem;
    out->Ji = g->Ji; out->Jj = g->Jj; out->Hd = g->Hd; out->fixed = g->fixed;
    return STBA_OK;
}
}  // namespace stba

// ---- coarse space: the sizes (pg_plan_coarse) and the buffers for a group size (lazily: the group size is an option of the solve)
static int pg_setup_coarse(stba_pg* g, int group_opt) {
    PgCoarsePlan plan;
    std::string why;
    const int rc = pg_plan_coarse(g->n, g->node_start_host, group_opt, &plan, &why);
    if (rc != 0) return fail(rc, why);
    if (plan.agg < 0) { g->coarse.agg = -1; g->coarse_valid = false; return STBA_OK; }
    if (plan.agg == g->coarse.agg) return STBA_OK;
    const int na = plan.na, nc = plan.nc, np = plan.np, parts = plan.parts;
    if (g->st2) STBA_HIP(hipStreamSynchronize(g->st2));       // (a job of the last solve may still be writing W / an inverse)
    g->job_in_flight = false;
    for (auto* buf : {&g->AdP, &g->Ac0, &g->W, &g->Ainv, &g->Ainv2, &g->inv_work, &g->rc_part, &g->zc, &g->part_cz, &g->Dc}) buf->reset();
    g->coarse.agg = 0;
    STBA_TRY(g->AdP.alloc((size_t)g->n * 36)); STBA_TRY(g->Ac0.alloc((size_t)nc * nc)); STBA_TRY(g->W.alloc((size_t)4 * np * np));
    STBA_TRY(g->Ainv.alloc((size_t)nc * nc)); STBA_TRY(g->Ainv2.alloc((size_t)nc * nc)); STBA_TRY(g->Dc.alloc((size_t)na * 36)); STBA_TRY(g->inv_work.alloc(chol_spd_inverse_workspace_doubles(np)));
    STBA_TRY(g->rc_part.alloc((size_t)na * parts * 6)); STBA_TRY(g->zc.alloc((size_t)nc)); STBA_TRY(g->part_cz.alloc((size_t)((nc + 3) / 4) * 2 + 2));
    STBA_HIP(hipMemsetAsync(g->rc_part, 0, (size_t)na * parts * 6 * sizeof(double), g->st));
    static DeviceOnce attr;
    STBA_TRY(attr.run([]() -> int {
        STBA_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(pg_coarse_build_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)PG_COARSE_BUILD_LDS_MAX));
        return STBA_OK;
    }));
    g->coarse = plan;
    g->coarse_valid = false;
    return STBA_OK;
}

// the second stream of the coarse inverse and its events (stba_pg_solve, coarse_async)
static int pg_second_stream(stba_pg* g) {
    if (g->st2) return STBA_OK;
    STBA_HIP(hipStreamCreateWithFlags(&g->st2, hipStreamNonBlocking));
    STBA_HIP(hipEventCreateWithFlags(&g->ev_in, hipEventDisableTiming));
    STBA_HIP(hipEventCreateWithFlags(&g->ev_read, hipEventDisableTiming));
    for (auto& e : g->ev_job) STBA_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    return STBA_OK;
}

// the first stream waits for an event of the second one only if the event has NOT fired yet when the dependent work is enqueued: a
// wait packet costs ~10 us of idle GPU even when its event has long fired (dense_chol.hip's note on the same), and here it nearly
// always has -- the job it guards started a whole PCG solve earlier.  The data flow is the same either way: same bits.
static int pg_wait_if_pending(hipStream_t st, hipEvent_t ev) {
    const hipError_t q = hipEventQuery(ev);
    if (q == hipSuccess) return STBA_OK;
    if (q != hipErrorNotReady) { (void)hipGetLastError(); }
    STBA_HIP(hipStreamWaitEvent(st, ev, 0));
    return STBA_OK;
}

// ---- stba_pg_solve's steps.  PgSolve is the state of ONE call; what outlives a call (job_in_flight, job_reads_pending, bend_valid,
// ac0_valid, coarse_valid, pp_base, pp_disabled, seq) stays in stba_pg.  No step captures anything; every launch is written once.
namespace {
struct PgSolve {
    stba_lm_options opt;
    stba_pcg_options pcg;
    // derived once
    bool coarse = false, async_inv = false, build_on_st2 = false, multi = false, forcing = false, pp_ok = false, timing = false;
    int chunk = 1;
    // the loop
    TrustRegion region;
    double cost = 0.0, gmax = 0.0, g2 = 0.0, eta = 0.0;
    double last_rel_decrease = 1.0;      // of the last accepted step: (cost before - cost after) / cost before
    int iter = 0, jobs = 0, since_refresh = 0;
    bool scale_init = false;
    bool head_done = false;              // the preconditioner and the job's head of the NEXT iteration are already on their way
    stba_pcg_summary ps;
    PgSolve(const stba_lm_options& o, const stba_pcg_options& p) : opt(o), pcg(p), region(o) { memset(&ps, 0, sizeof ps); }
};

// the rest of a second-stream job, for whoever enqueues it: the buffer of the pair it writes, and whether its head is already out
struct PgJob { int wbuf = 0; bool head_was_done = false; };
// what pg_coarse_refresh leaves to the iteration: the inverse its PCG reads, and a job that is still to be enqueued
struct PgCoarseUse { const double* Ainv = nullptr; bool job_deferred = false; PgJob job; };

void pg_precond(stba_pg* g, PgSolve& sv) {
    hipLaunchKernelGGL(pg_precond_kernel, dim3(g->nb_nodes), dim3(256), 0, g->st, g->n, g->Hd, g->scale, sv.scale_init ? 0 : 1,
                       sv.opt.jacobi_scaling, sv.region.radius, sv.opt.min_lm_diagonal, sv.opt.max_lm_diagonal, g->fixed, g->d, g->Minv);
    sv.scale_init = true;
}

void pg_offdiag_if_stale(stba_pg* g) {
    if (g->bend_valid) return;
    hipLaunchKernelGGL(pg_offdiag_kernel, dim3(g->nb_edges), dim3(256), 0, g->st, g->m, g->Ji, g->Jj, g->end_pos, g->Bend);
    g->bend_valid = true;
}

// the coarse matrix P^T J^T J P from the blocks; add_nodes: with the diagonal blocks' part (several ranks: rank 0 alone)
void pg_coarse_build(stba_pg* g, hipStream_t st, int add_nodes) {
    hipLaunchKernelGGL(pg_coarse_build_kernel, dim3(g->coarse.na), dim3(256), g->coarse.build_lds_bytes, st, g->n, g->coarse.agg, g->coarse.nc,
                       add_nodes, g->node_start, g->end_node, g->end_rem, g->Bend, g->Hd, g->AdP, g->Ac0);
}

// its damping term P^T D P, and W = the padded sum of the two
void pg_coarse_damped(stba_pg* g, hipStream_t st) {
    const size_t cnt = (size_t)3 * g->coarse.np * g->coarse.np;
    hipLaunchKernelGGL(pg_coarse_dc_kernel, dim3(g->coarse.na), dim3(256), 0, st, g->n, g->coarse.agg, g->AdP, g->d, g->Dc);
    hipLaunchKernelGGL(pg_coarse_assemble_kernel, dim3((unsigned)((cnt + 255) / 256)), dim3(256), 0, st, g->coarse.nc, g->coarse.np, g->Ac0, g->Dc, g->W);
}

// W^-1 -> Aout
int pg_coarse_invert(stba_pg* g, hipStream_t st, double* Aout) {
    STBA_TRY(chol_spd_inverse_dev(g->W, 2 * g->coarse.np, g->coarse.np, g->coarse.nc, g->cflag, g->inv_work, st));
    hipLaunchKernelGGL(pg_coarse_finish_kernel, dim3((unsigned)(((size_t)g->coarse.nc * g->coarse.nc + 255) / 256)), dim3(256), 0, st, g->coarse.nc, g->coarse.np, g->W, Aout,
                       g->cflag, g->cflag + 1);
    return STBA_OK;
}

// the tail of the two finish kernels.  One rank: the kernel has written the stamped block itself.  Several: it wrote g->scal_dev, the
// hook sums the first n_summed scalars and a kernel exports the n_payload of them with the stamp.  Then the host reads g->fin_vals.
int pg_read_block(stba_pg* g, int n_summed, int n_payload) {
    if (g->ar) {
        STBA_TRY(pg_hook(g, g->scal_dev, (size_t)n_summed));
        hipLaunchKernelGGL(pg_export_kernel, dim3(1), dim3(64), 0, g->st, n_payload, g->scal_dev, g->fin.dev, g->seq);
    }
    STBA_HIP(hipGetLastError());
    const double seq = g->seq;
    return stamped_wait(g->fin.host, n_payload, [seq](double st) { return st == seq; }, g->fin_vals, hip_stream_state(g->st), "pose graph", 120.0);
}

// (the job of the second stream reads the blocks, the coarse basis and the damping of the linearisation it belongs to: whatever
// overwrites them -- the next linearisation, or the preconditioner kernel -- waits until it has: an event that has long fired by then)
int pg_wait_for_job_reads(stba_pg* g) {
    if (g->job_reads_pending) { STBA_TRY(pg_wait_if_pending(g->st, g->ev_read)); g->job_reads_pending = false; }
    return STBA_OK;
}

// the PCG solve as one kernel: one rank, a coarse space whose groups fit a workgroup (<= 64 nodes, all their edge-end products
// in LDS) and are all resident at once (one per CU)
bool pg_one_kernel_eligible(stba_pg* g, const PgSolve& sv) {
    // the clauses that need no device first: a solve they rule out (several ranks, one_kernel_solve = 0, no coarse space) asks it nothing
    if (!pg_one_kernel_fits(g->coarse, sv.pcg.one_kernel_solve, sv.multi, PgDeviceLimits{INT_MAX, INT_MAX})) return false;
    // (the compute units, and the LDS a workgroup may opt in to, are properties of the device and the driver: asked, not assumed --
    // advisor, round 5)
    int dev = 0;
    PgDeviceLimits lim{0, 0};
    bool pp_ok = hipGetDevice(&dev) == hipSuccess && hipDeviceGetAttribute(&lim.cus, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess &&
                 hipDeviceGetAttribute(&lim.lds_max_optin, hipDeviceAttributeMaxSharedMemoryPerBlock, dev) == hipSuccess &&
                 pg_one_kernel_fits(g->coarse, sv.pcg.one_kernel_solve, sv.multi, lim);
    if (pp_ok) {
        static DeviceOnce attr;
        // a device that refuses the attribute takes the launch path; that is not a failed solve
        if (attr.run([]() -> int {
                STBA_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(pg_pcg_persistent_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)PP_LDS_MAX));
                return STBA_OK;
            }) != STBA_OK) { pp_ok = false; g->pp_disabled = true; (void)hipGetLastError(); }
    }
    return pp_ok;
}

// ---- set-up of a solve: the coarse space for this group size, the second stream, the flags derived once
int pg_solve_begin(stba_pg* g, PgSolve& sv) {
    const stba_pcg_options& pcg = sv.pcg;
    STBA_TRY(pg_setup_coarse(g, pcg.coarse_group));
    sv.coarse = g->coarse.agg > 0;
    // the second stream of the coarse inverse (pg_coarse_refresh); a job of the previous solve may still be in flight: it is awaited here,
    // where it costs nothing, instead of at the end of that solve, where it would have been the last 0.3 ms of its wall time
    sv.async_inv = sv.coarse && pcg.coarse_async != 0;
    if (sv.async_inv) {
        STBA_TRY(pg_second_stream(g));
        if (g->job_in_flight) { STBA_HIP(hipStreamSynchronize(g->st2)); g->job_in_flight = false; }
        g->job_reads_pending = false;
    }
    sv.build_on_st2 = sv.async_inv && !g->ar;
    if (sv.coarse) STBA_HIP(hipMemsetAsync(g->cflag + 1, 0, sizeof(int), g->st));      // this solve's count of failed coarse operators
    sv.multi = (g->ar != nullptr);
    sv.chunk = std::max(1, pcg.check_every);
    sv.forcing = pcg.forcing_eta0 > 0.0;
    sv.eta = pcg.forcing_eta0;
    sv.ps.coarse_dim = sv.coarse ? g->coarse.nc : 0;
    sv.pp_ok = pg_one_kernel_eligible(g, sv);
    // (stba_lm_options::phase_timing: hipEvents around the linear solve -- the persistent kernel, or the launches of the PCG loop --
    // for bench.py's roofline of the C4 line; an event is a packet of its own on the queue, so only on request)
    sv.timing = sv.opt.phase_timing != 0;
    return STBA_OK;
}

// ---- linearisation at the current point: residuals, Jacobians, gradient | diagonal blocks, the coarse basis and matrix
int pg_linearize_enqueue(stba_pg* g, const PgSolve& sv) {
    STBA_TRY(pg_wait_for_job_reads(g));
    STBA_TRY(pg_linearize(g, g->cur, true));
    pg_gather_blocks(g);
    STBA_TRY(pg_hook(g, g->g, (size_t)g->n * 42));
    hipLaunchKernelGGL(pg_gnorm_kernel, dim3(g->nb_vec), dim3(256), 0, g->st, 6 * g->n, g->g, g->part_c);
    if (sv.coarse) {
        hipLaunchKernelGGL(pg_coarse_basis_kernel, dim3(g->nb_nodes), dim3(256), 0, g->st, g->n, g->coarse.agg, g->poses[g->cur], g->fixed, g->AdP);
        pg_offdiag_if_stale(g);
        // (one rank with the coarse inverse on its second stream: the coarse MATRIX is only read by that job, and is built there --
        // 55 us of every LM iteration off the critical path; several ranks sum it with the hook, on the engine's stream)
        if (!sv.build_on_st2) {
            pg_coarse_build(g, g->st, (!g->ar || g->rank == 0) ? 1 : 0);
            STBA_TRY(pg_hook(g, g->Ac0, (size_t)g->coarse.nc * g->coarse.nc));
        }
        g->coarse_valid = false;
        g->ac0_valid = false;
    }
    STBA_HIP(hipGetLastError());
    return STBA_OK;
}

// cost and |g|_inf of that linearisation: one kernel sums, the host reads mapped memory (several ranks: the cost goes over the hook)
int pg_linearize_finish(stba_pg* g, double* cost, double* gmax, double* g2) {
    g->seq += 1.0;
    hipLaunchKernelGGL(pg_linear_finish_kernel, dim3(1), dim3(256), 0, g->st, g->nb_edges, g->part_e, g->nb_vec, g->part_c, g->ar ? g->scal_dev : g->fin.dev, g->seq);
    STBA_TRY(pg_read_block(g, 1, 3));
    *cost = 0.5 * g->fin_vals[0]; *gmax = g->fin_vals[1]; *g2 = g->fin_vals[2];
    return STBA_OK;
}

// the HEAD of the second stream's job (one rank): everything the inverse needs -- the coarse matrix from the blocks, the diagonal
// blocks and the basis of THIS linearisation, its damping term, the workspace; READ_k tells the first stream when its next
// linearisation / preconditioner kernel may overwrite those inputs.  Three launches: behind an accepted step they are enqueued
// at once (the preconditioner kernel in front of them), so that they run under the host's wait for the new point's scalars
// instead of at the start of the PCG kernel, with which the inversion then competes for CUs.
int pg_job_head(stba_pg* g) {
    STBA_HIP(hipStreamWaitEvent(g->st2, g->ev_in, 0));
    if (!g->ac0_valid) {
        pg_coarse_build(g, g->st2, 1);
        g->ac0_valid = true;
    }
    pg_coarse_damped(g, g->st2);
    STBA_HIP(hipEventRecord(g->ev_read, g->st2));
    g->job_reads_pending = true;
    g->job_in_flight = true;
    return STBA_OK;
}

// THE JOB: ~ 30 launches on the second stream.  Enqueueing them takes the HOST ~ 250 us -- so when the iteration does not
// wait for them (the usual case), the PCG kernel is launched FIRST and the job is enqueued while it runs: with the job in
// front, the kernel timeline showed the first stream idle for 277 us of every 760 us iteration, waiting for the host
// (profiles/r6_c4_iter_trace.txt)
int pg_job_rest(stba_pg* g, const PgSolve& sv, const PgJob& job) {
    if (!job.head_was_done) { if (sv.build_on_st2) STBA_TRY(pg_job_head(g)); else STBA_HIP(hipStreamWaitEvent(g->st2, g->ev_in, 0)); }
    STBA_TRY(pg_coarse_invert(g, g->st2, job.wbuf ? g->Ainv2 : g->Ainv));
    STBA_HIP(hipEventRecord(g->ev_job[job.wbuf], g->st2));
    g->job_in_flight = true;
    return STBA_OK;
}

// ---- coarse operator (P^T (J^T J + D) P)^-1 of an LM iteration
int pg_coarse_refresh(stba_pg* g, PgSolve& sv, bool head_was_done, PgCoarseUse* use) {
    use->Ainv = g->Ainv;
    use->job_deferred = false;
    if (sv.coarse && sv.async_inv) {
        // ROUND 6: off the critical path.  The inversion (eight panels of a ~45 us chain on a handful of CUs: 0.39 of a 0.92 ms LM
        // iteration at C4) runs on a SECOND stream, next to this iteration's PCG kernel (157 workgroups on 256 CUs), and is applied one LM
        // iteration LATE: iteration k preconditions with the inverse of iteration k - 1's operator -- an inverse made at the
        // previous linearisation / damping still is a preconditioner, only a weaker one (coarse_refresh_every = 2 had measured
        // + 9 % PCG iterations).  The very first solve has no predecessor: it waits for its own inverse (coarse_async = 2 with a
        // forcing sequence: it runs on block Jacobi alone, Ainv = 0 -- 3 PCG iterations at eta_0 = 0.1, but a first step that
        // leaves the cost at 1021 where the two-level step leaves 258 and the exact one 48: the whole trajectory moves).
        // Everything is ordered by events, so the result does not depend on timing: run to run the same bits.
        //   stream 1: precond_k | wait job_{k-1} | record IN_k | PCG_k (Ainv of job_{k-1}) | trial | wait READ_k | linearise ...
        //   stream 2:                              wait IN_k   | coarse matrix, Dc_k, assemble W_k | record READ_k | invert -> Ainv[k & 1] | record job_k
        // (several ranks: coarse matrix -- summed by the hook --, Dc_k and W_k stay on stream 1, IN_k is recorded behind them)
        const int wbuf = sv.jobs & 1;
        double* Aw = wbuf ? g->Ainv2 : g->Ainv;
        double* Ar = wbuf ? g->Ainv : g->Ainv2;        // written by the previous job (or zeroed below)
        if (sv.jobs == 0) STBA_HIP(hipMemsetAsync(Ar, 0, (size_t)g->coarse.nc * g->coarse.nc * sizeof(double), g->st));
        else STBA_TRY(pg_wait_if_pending(g->st, g->ev_job[(sv.jobs - 1) & 1]));
        const bool own = pg_waits_for_own_inverse(sv.pcg, sv.forcing, sv.jobs, sv.iter, sv.last_rel_decrease);
        if (!sv.build_on_st2) pg_coarse_damped(g, g->st);
        if (!head_was_done) STBA_HIP(hipEventRecord(g->ev_in, g->st));
        use->job.wbuf = wbuf;
        use->job.head_was_done = head_was_done;
        use->Ainv = Ar;
        if (own) {
            STBA_TRY(pg_job_rest(g, sv, use->job));
            STBA_HIP(hipStreamWaitEvent(g->st, g->ev_job[wbuf], 0));
            use->Ainv = Aw;
        } else use->job_deferred = true;
        ++sv.jobs;
        g->coarse_valid = true;
        ++sv.ps.coarse_refreshes;
    } else if (sv.coarse && (sv.ps.coarse_refreshes < 2 || sv.since_refresh >= std::max(1, sv.pcg.coarse_refresh_every))) {
        // (synchronous form, coarse_async = 0) rebuilt when the linearisation or (every coarse_refresh_every-th time) the damping changed
        // (the inverse is a preconditioner: one made at an earlier linearisation / damping still is one, only weaker -- with
        // coarse_refresh_every = k it is re-made every k-th LM iteration; the first two iterations always make theirs)
        pg_coarse_damped(g, g->st);
        STBA_TRY(pg_coarse_invert(g, g->st, g->Ainv));
        g->coarse_valid = true;
        sv.since_refresh = 0;
        ++sv.ps.coarse_refreshes;
    }
    ++sv.since_refresh;
    return STBA_OK;
}

// ---- PCG on (J^T J + D) x = -g, stopped on the device at |r| <= eta_k |g|: four launches per iteration, watched by the host
int pg_pcg_by_launches(stba_pg* g, const PgSolve& sv, const double* Ainv_use, double eta_k) {
    const stba_pcg_options& pcg = sv.pcg;
    const bool coarse = sv.coarse;
    const double* AdP = coarse ? g->AdP : nullptr;
    // (every kernel of the previous solve has finished -- the host has read the trial block behind them -- so the exported
    // block can be taken back: the wait below must not see the previous solve's tick count and `done`)
    g->exp.zero();
    std::atomic_thread_fence(std::memory_order_seq_cst);
    hipLaunchKernelGGL(pg_pcg_init4_kernel, dim3(g->nb_nodes4), dim3(PG_NT), 0, g->st, g->n, g->coarse.agg, g->g, g->Minv, AdP, g->x, g->rr, g->z,
                       g->rc_part, g->part_a);
    if (coarse)
        hipLaunchKernelGGL(pg_coarse_solve_kernel, dim3((g->coarse.nc + 3) / 4), dim3(256), 0, g->st, g->coarse.nc, g->coarse.parts, (const PgPcgState*)nullptr, Ainv_use, g->rc_part,
                           g->zc, g->part_cz);
    hipLaunchKernelGGL(pg_pcg_dir4_kernel, dim3(g->nb_nodes4), dim3(PG_NT), 0, g->st, g->n, g->coarse.agg, 1, 1, eta_k, pcg.max_iterations, g->state, g->exp.dev,
                       g->nb_nodes4, g->part_a, (g->coarse.nc + 3) / 4, coarse ? g->part_cz : nullptr, AdP, g->zc, g->z, g->d, g->p, g->part_d);
    STBA_HIP(hipGetLastError());
    int enq = 0;
    bool pcg_done = false;
    double px[PX_COUNT];
    STBA_TRY(stamped_wait(g->exp.host, PX_COUNT, [](double st) { return st >= 1.0; }, px, hip_stream_state(g->st), "pose graph",
                          120.0));          // (also: the previous solve's ticks are gone)
    if (px[PX_DONE] != 0.0) pcg_done = true;
    while (!pcg_done && enq < pcg.max_iterations) {
        const int todo = std::min(sv.chunk, pcg.max_iterations - enq);
        for (int c = 0; c < todo; ++c, ++enq) {
            const int slot = enq & 1;
            if (!sv.multi) {
                hipLaunchKernelGGL(pg_edge_product_kernel, dim3(g->nb_edges), dim3(256), 0, g->st, g->m, g->ei, g->ej, g->Ji, g->Jj, g->p, g->u,
                                   g->part_c, g->state);
                hipLaunchKernelGGL(pg_pcg_update4_kernel<true>, dim3(g->nb_nodes4), dim3(PG_NT), 0, g->st, g->n, g->m, g->coarse.agg, slot, g->state, g->nb_edges,
                                   g->part_c, g->nb_nodes4, g->part_d, g->Minv, AdP, g->d, g->node_start, g->end_code, g->u, (const double*)nullptr,
                                   g->p, g->x, g->rr, g->z, g->rc_part, g->part_a);
            } else {
                STBA_TRY(pg_apply(g, g->p, g->q, true));
                hipLaunchKernelGGL(pg_dot_kernel, dim3(g->nb_vec), dim3(256), 0, g->st, 6 * g->n, g->p, g->q, g->part_c);
                hipLaunchKernelGGL(pg_pcg_update4_kernel<false>, dim3(g->nb_nodes4), dim3(PG_NT), 0, g->st, g->n, g->m, g->coarse.agg, slot, g->state, g->nb_vec,
                                   g->part_c, 0, (const double*)nullptr, g->Minv, AdP, g->d, g->node_start, g->end_code, g->u, g->q,
                                   g->p, g->x, g->rr, g->z, g->rc_part, g->part_a);
            }
            if (coarse)
                hipLaunchKernelGGL(pg_coarse_solve_kernel, dim3((g->coarse.nc + 3) / 4), dim3(256), 0, g->st, g->coarse.nc, g->coarse.parts, g->state, Ainv_use, g->rc_part, g->zc,
                                   g->part_cz);
            hipLaunchKernelGGL(pg_pcg_dir4_kernel, dim3(g->nb_nodes4), dim3(PG_NT), 0, g->st, g->n, g->coarse.agg, slot, 0, eta_k, pcg.max_iterations, g->state,
                               g->exp.dev, g->nb_nodes4, g->part_a, (g->coarse.nc + 3) / 4, coarse ? g->part_cz : nullptr, AdP, g->zc, g->z, g->d, g->p, g->part_d);
        }
        STBA_HIP(hipGetLastError());
        // one rank: the host looks at the chunk BEFORE the one it has just enqueued (the stream never runs dry; the kernels of a
        // chunk enqueued past convergence return at once).  Several ranks: every rank must enqueue the same collectives, so the
        // decision waits for the chunk itself -- the solve state is replicated and every rank sees the same `done`.
        const double want = 1 + (sv.multi ? enq : enq - todo);
        STBA_TRY(stamped_wait(g->exp.host, PX_COUNT, [want](double st) { return st >= want; }, px, hip_stream_state(g->st), "pose graph",
                              120.0));
        if (px[PX_DONE] != 0.0) pcg_done = true;
    }
    return STBA_OK;
}

// the same solve as ONE kernel (see pg_pcg_persistent_kernel): nothing for the host to watch, the trial point follows on the stream
int pg_pcg_one_kernel(stba_pg* g, const PgSolve& sv, const double* Ainv_use, double eta_k) {
    const stba_pcg_options& pcg = sv.pcg;
    pg_offdiag_if_stale(g);
    if (g->pp_base > (1 << 30)) {        // (stamps only grow; long before they wrap they are taken back to zero)
        STBA_HIP(hipMemsetAsync(g->ustamp, 0, PP_GROUPS_MAX * PP_STAMP * sizeof(int), g->st));
        STBA_HIP(hipMemsetAsync(g->pstamp, 0, PP_GROUPS_MAX * PP_STAMP * sizeof(int), g->st));
        g->pp_base = 0;
    }
    PpArgs a;
    a.n = g->n; a.agg = g->coarse.agg; a.log2agg = 0; while ((1 << a.log2agg) < g->coarse.agg) ++a.log2agg;
    a.na = g->coarse.na; a.nc = g->coarse.nc; a.base = g->pp_base; a.max_iters = pcg.max_iterations; a.eta = eta_k;
    a.node_start = g->node_start; a.end_rem = g->end_rem; a.Bend = g->Bend; a.Hd = g->Hd; a.d = g->d; a.Minv = g->Minv; a.AdP = g->AdP;
    a.Ainv = Ainv_use; a.g = g->g; a.x = g->x; a.ubuf = g->ubuf; a.pbuf = g->pbuf; a.ustamp = g->ustamp; a.pstamp = g->pstamp;
    a.state = g->state; a.spin_limit = pcg.one_kernel_solve == 2 ? 0 : 25000000ll;      // (a quarter of a second of wall_clock64 ticks; 2: the test of the way back)
    a.fences = pcg.one_kernel_solve == 3 ? 1 : 0;
    a.eta_c = sv.forcing ? pcg.coarse_eta : 0.0;
    a.tdbg = nullptr;
#ifdef STBA_DEBUG_KNOBS
    static long long* tdbg_dev = nullptr;
    if (knob_int("STBA_PP_TIMING", 0)) {
        if (!tdbg_dev) { STBA_HIP(hipMalloc(&tdbg_dev, 8 * sizeof(long long))); STBA_HIP(hipMemset(tdbg_dev, 0, 8 * sizeof(long long))); }
        a.tdbg = tdbg_dev;
    }
#endif
    hipLaunchKernelGGL(pg_pcg_persistent_kernel, dim3(g->coarse.na), dim3(PP_T), pp_lds_bytes(g->coarse.na, g->coarse.nc), g->st, a);
#ifdef STBA_DEBUG_KNOBS
    if (a.tdbg) {
        long long h[8];
        STBA_HIP(hipMemcpyAsync(h, tdbg_dev, sizeof h, hipMemcpyDeviceToHost, g->st)); STBA_HIP(hipStreamSynchronize(g->st));
        fprintf(stderr, "pp phases (x 10 ns, cumulative): publish %lld | ends %lld | w+sum9 %lld | all-gather %lld | scalars+update %lld | coarse+u %lld | loop top %lld\n",
                h[0], h[1], h[2], h[3], h[4], h[5], h[6]);
    }
#endif
    STBA_HIP(hipGetLastError());
    g->pp_base += pcg.max_iterations + 8;
    return STBA_OK;
}

// ---- model change, trial point: |J x|^2 from the edge kernel (its |t_e|^2 sums), g.x and the step norms from the update kernel;
// the trial block (cost, x^T H x, g.x, |step|^2, |x|^2, PCG iterations, capped / timed out, |r_0|^2) comes home in g->fin_vals
int pg_trial_point(stba_pg* g) {
    const int nxt = g->cur ^ 1;
    hipLaunchKernelGGL(pg_edge_product_kernel, dim3(g->nb_edges), dim3(256), 0, g->st, g->m, g->ei, g->ej, g->Ji, g->Jj, g->x, g->u, g->part_b,
                       (const PgPcgState*)nullptr);
    hipLaunchKernelGGL(pg_update4_kernel, dim3(g->nb_nodes), dim3(256), 0, g->st, g->n, g->poses[g->cur], g->x, g->g, g->fixed, g->poses[nxt], g->part_u);
    STBA_TRY(pg_linearize(g, nxt, false));
    g->seq += 1.0;
    hipLaunchKernelGGL(pg_trial_finish_kernel, dim3(1), dim3(256), 0, g->st, g->nb_edges, g->part_e, g->nb_edges, g->part_b, g->nb_nodes, g->part_u,
                       g->state, g->ar ? g->scal_dev : g->fin.dev, g->seq);
    return pg_read_block(g, 2, 8);      // (several ranks: cost and |J x|^2 summed over the edge shards)
}
}  // namespace

extern "C" {

void stba_pcg_default_options(stba_pcg_options* o) {
    if (!o) return;
    o->max_iterations = 1000;
    o->relative_tolerance = 1e-12;
    o->check_every = 4;
    o->forcing_eta0 = 0.1;
    o->forcing_eta_min = 0.01;          // (stba.h: the measured reason)
    o->coarse_group = 0;
    o->coarse_refresh_every = 1;
    o->one_kernel_solve = 1;
    o->coarse_async = 1;
    o->forcing_eta_final = 0.0;
    o->coarse_eta = 0.0;
    o->coarse_async_after = 1;
    o->coarse_async_decrease = 0.5;
}

// everything of stba_pg_create behind the engine object and its stream: the buffers and their contents.  A failure leaves a partly
// filled engine, which stba_pg_create frees
static int pg_fill(stba_pg* g, int n_nodes, int n_edges, const double* poses, const int* edge_i, const int* edge_j, const double* meas,
                   const unsigned char* node_fixed) {
    const size_t n = (size_t)n_nodes, m = (size_t)n_edges;
    STBA_TRY(g->poses[0].alloc(n * 7)); STBA_TRY(g->poses[1].alloc(n * 7)); STBA_TRY(g->ei.alloc(m)); STBA_TRY(g->ej.alloc(m));
    STBA_TRY(g->meas.alloc(m * 7)); STBA_TRY(g->r.alloc(m * 6)); STBA_TRY(g->Ji.alloc(m * 36)); STBA_TRY(g->Jj.alloc(m * 36));
    STBA_TRY(g->g.alloc(n * 42)); g->Hd = g->g + n * 6;      // [gradient 6n | diagonal blocks 36n]: one cross-rank sum
    STBA_TRY(g->Minv.alloc(n * 36)); STBA_TRY(g->d.alloc(n * 6)); STBA_TRY(g->scalar.alloc(1));
    STBA_TRY(g->scale.alloc(n * 6)); STBA_TRY(g->x.alloc(n * 6)); STBA_TRY(g->rr.alloc(n * 6)); STBA_TRY(g->z.alloc(n * 6));
    STBA_TRY(g->p.alloc(n * 6)); STBA_TRY(g->q.alloc(n * 6));
    const size_t np_ = (size_t)std::max(g->nb_vec, std::max(g->nb_nodes, g->nb_edges)) * 2 + 2;
    STBA_TRY(g->part_e.alloc(np_)); STBA_TRY(g->part_a.alloc(np_)); STBA_TRY(g->part_b.alloc(np_)); STBA_TRY(g->part_c.alloc(np_));
    STBA_TRY(g->part_d.alloc(np_));
    if (node_fixed) STBA_TRY(g->fixed.alloc(n));
    STBA_TRY(g->node_start.alloc(n + 1)); STBA_TRY(g->end_code.alloc(2 * m)); STBA_TRY(g->u.alloc(12 * m));
    STBA_TRY(g->end_node.alloc(2 * m)); STBA_TRY(g->contrib.alloc(2 * m * 28));
    STBA_TRY(g->end_pos.alloc(2 * m)); STBA_TRY(g->end_rem.alloc(2 * m)); STBA_TRY(g->Bend.alloc(72 * m)); STBA_TRY(g->ubuf.alloc(12 * n));
    STBA_TRY(g->pbuf.alloc((size_t)2 * PP_GROUPS_MAX * PP_SLOT)); STBA_TRY(g->ustamp.alloc((size_t)PP_GROUPS_MAX * PP_STAMP)); STBA_TRY(g->pstamp.alloc((size_t)PP_GROUPS_MAX * PP_STAMP));
    if (hipMemsetAsync(g->ustamp, 0, PP_GROUPS_MAX * PP_STAMP * sizeof(int), g->st) != hipSuccess ||
        hipMemsetAsync(g->pstamp, 0, PP_GROUPS_MAX * PP_STAMP * sizeof(int), g->st) != hipSuccess)
        return fail(STBA_ERR_HIP, "stba_pg_create: memset");
    g->nb_nodes4 = (n_nodes + PG_NPW - 1) / PG_NPW;
    STBA_TRY(g->part_u.alloc((size_t)g->nb_nodes * 4 + 4)); STBA_TRY(g->scal_dev.alloc(16)); STBA_TRY(g->state.alloc(1)); STBA_TRY(g->cflag.alloc(2));
    if (g->exp.alloc((size_t)stamped_doubles(PX_COUNT)) != STBA_OK || g->fin.alloc(16) != STBA_OK)
        return fail(STBA_ERR_ALLOC, "stba_pg_create: mapped host memory");
    memset(&g->last_pcg, 0, sizeof g->last_pcg);
    {   // the edge ends sorted by node (pg_plan.hpp)
        PgEnds ends;
        pg_build_ends(n_nodes, n_edges, edge_i, edge_j, &ends);
        if (upload(g->end_pos, ends.end_pos.data(), 2 * m, g->st) != STBA_OK || upload(g->end_rem, ends.end_rem.data(), 2 * m, g->st) != STBA_OK ||
            upload(g->node_start, ends.node_start.data(), n + 1, g->st) != STBA_OK || upload(g->end_code, ends.end_code.data(), 2 * m, g->st) != STBA_OK ||
            upload(g->end_node, ends.end_node.data(), 2 * m, g->st) != STBA_OK || hipStreamSynchronize(g->st) != hipSuccess)
            return fail(STBA_ERR_HIP, "stba_pg_create: upload failed");
        g->node_start_host.swap(ends.node_start);
    }
    if (upload(g->poses[0], poses, n * 7, g->st) != STBA_OK || upload(g->ei, edge_i, m, g->st) != STBA_OK ||
        upload(g->ej, edge_j, m, g->st) != STBA_OK || upload(g->meas, meas, m * 7, g->st) != STBA_OK ||
        (node_fixed && upload(g->fixed, node_fixed, n, g->st) != STBA_OK) || hipStreamSynchronize(g->st) != hipSuccess)
        return fail(STBA_ERR_HIP, "stba_pg_create: upload failed");
    // The buffers of the default coarse space, the second stream and its events are made HERE (round 6): a solve used to begin with
    // a dozen allocations (the 33 MB inversion workspace among them), a stream and four events -- ~ 0.4 ms of a 6.4 ms C4 solve
    // on a fresh engine, inside the time every caller and bench.py measure.  (A solve with another group size makes its own; a
    // graph too large for the default space is told so by the solve, not here.)
    if (pg_setup_coarse(g, 0) == STBA_OK && g->coarse.agg > 0) (void)pg_second_stream(g);
    (void)hipStreamSynchronize(g->st);
    return STBA_OK;
}

int stba_pg_create(stba_pg** out, int n_nodes, int n_edges, const double* poses, const int* edge_i, const int* edge_j,
                   const double* meas, const unsigned char* node_fixed, void* hip_stream) {
    if (!out) return fail(STBA_ERR_INVALID_ARGUMENT, "out is null");
    *out = nullptr;
    if (n_nodes <= 0 || n_edges <= 0 || !poses || !edge_i || !edge_j || !meas)
        return fail(STBA_ERR_INVALID_ARGUMENT, "stba_pg_create: null or empty input");
    if (pg_check_edges(n_nodes, n_edges, edge_i, edge_j) >= 0) return fail(STBA_ERR_INVALID_ARGUMENT, "stba_pg_create: bad edge");
    STBA_TRY(require_device());
    stba_pg* g = new stba_pg();
    g->n = n_nodes; g->m = n_edges;
    g->h_ei.assign(edge_i, edge_i + n_edges); g->h_ej.assign(edge_j, edge_j + n_edges);
    if (node_fixed) g->h_fixed.assign(node_fixed, node_fixed + n_nodes);
    if (hip_stream) g->st = reinterpret_cast<hipStream_t>(hip_stream);
    else { if (hipStreamCreate(&g->st) != hipSuccess) { delete g; return fail(STBA_ERR_HIP, "hipStreamCreate"); } g->own = true; }
    g->nb_nodes = (n_nodes + 255) / 256; g->nb_vec = (6 * n_nodes + 255) / 256; g->nb_edges = (n_edges + 255) / 256;
    const int rc = pg_fill(g, n_nodes, n_edges, poses, edge_i, edge_j, meas, node_fixed);
    if (rc != STBA_OK) { pg_free(g); return rc; }
    *out = g;
    return STBA_OK;
}

int stba_pg_set_allreduce(stba_pg* g, stba_allreduce_fn fn, void* user, int rank, int world_size) {
    if (!g || rank < 0 || world_size < 1 || rank >= world_size) return fail(STBA_ERR_INVALID_ARGUMENT, "bad argument");
    if (!fn && world_size > 1) return fail(STBA_ERR_INVALID_ARGUMENT, "stba_pg_set_allreduce: world_size > 1 needs a hook");
    g->ar = (world_size > 1 || fn) ? fn : nullptr;
    g->ar_user = user; g->rank = rank; g->world = world_size;
    return STBA_OK;
}

int stba_pg_destroy(stba_pg* g) {
    if (!g) return STBA_OK;
    pg_free(g);
    return STBA_OK;
}

int stba_pg_get_poses(stba_pg* g, double* poses) {
    if (!g || !poses) return fail(STBA_ERR_INVALID_ARGUMENT, "null argument");
    STBA_HIP(hipMemcpyAsync(poses, g->poses[g->cur], (size_t)g->n * 7 * sizeof(double), hipMemcpyDeviceToHost, g->st));
    STBA_HIP(hipStreamSynchronize(g->st));
    return STBA_OK;
}

int stba_pg_evaluate(stba_pg* g, double* cost, double* r, double* Ji, double* Jj) {
    if (!g) return fail(STBA_ERR_INVALID_ARGUMENT, "null engine");
    STBA_TRY(pg_linearize(g, g->cur, true));
    std::vector<double> buf;
    double c2 = host_sum(g->st, g->part_e, g->nb_edges, 1, 0, buf);
    STBA_TRY(pg_sum_ranks(g, &c2));
    if (cost) *cost = 0.5 * c2;
    if (r) STBA_HIP(hipMemcpyAsync(r, g->r, (size_t)g->m * 6 * sizeof(double), hipMemcpyDeviceToHost, g->st));
    // (the device keeps the Jacobians component-major, [36][m]; the caller gets them edge-major, [m][6][6])
    std::vector<double> ti, tj;
    if (Ji) { ti.resize((size_t)g->m * 36); STBA_HIP(hipMemcpyAsync(ti.data(), g->Ji, ti.size() * sizeof(double), hipMemcpyDeviceToHost, g->st)); }
    if (Jj) { tj.resize((size_t)g->m * 36); STBA_HIP(hipMemcpyAsync(tj.data(), g->Jj, tj.size() * sizeof(double), hipMemcpyDeviceToHost, g->st)); }
    STBA_HIP(hipStreamSynchronize(g->st));
    for (int k = 0; k < 36; ++k)
        for (int e = 0; e < g->m; ++e) {
            if (Ji) Ji[(size_t)e * 36 + k] = ti[(size_t)k * g->m + e];
            if (Jj) Jj[(size_t)e * 36 + k] = tj[(size_t)k * g->m + e];
        }
    return STBA_OK;
}

// measurement (bench.py --config c4): hipEvent-timed averages of the two kernels a solve is made of -- the residual +
// Jacobian kernel and one matrix-free product q = (J^T J + D) p (diagonal term + edge kernel) -- on the engine's stream
int stba_pg_time_kernels(stba_pg* g, int reps, double* ms_linearize, double* ms_matvec) {
    if (!g || reps <= 0 || !ms_linearize || !ms_matvec) return fail(STBA_ERR_INVALID_ARGUMENT, "bad argument");
    hipEvent_t e0, e1, e2;
    STBA_HIP(hipEventCreate(&e0)); STBA_HIP(hipEventCreate(&e1)); STBA_HIP(hipEventCreate(&e2));
    STBA_TRY(pg_linearize(g, g->cur, true));            // warm-up; also makes the Jacobians the products use
    // (a non-zero direction and damping -- the gradient of this linearisation, unit damping -- so that the product does the
    // atomics a real one does)
    STBA_HIP(hipMemsetAsync(g->g, 0, (size_t)g->n * 42 * sizeof(double), g->st));
    hipLaunchKernelGGL(pg_accumulate_kernel, dim3((2 * g->m + 255) / 256), dim3(256), 0, g->st, g->m, g->ei, g->ej, g->r, g->Ji, g->Jj, g->g, g->Hd);
    STBA_HIP(hipMemcpyAsync(g->p, g->g, (size_t)6 * g->n * sizeof(double), hipMemcpyDeviceToDevice, g->st));
    STBA_HIP(hipMemcpyAsync(g->d, g->g, (size_t)6 * g->n * sizeof(double), hipMemcpyDeviceToDevice, g->st));
    // the product as the one-rank solve runs it: the edge kernel (t_e, u_e = J_e^T t_e, |t_e|^2) -- the node kernel gathers u
    // while it updates x, r, z and is not a product kernel of its own
    int rc = STBA_OK;
    hipLaunchKernelGGL(pg_edge_product_kernel, dim3(g->nb_edges), dim3(256), 0, g->st, g->m, g->ei, g->ej, g->Ji, g->Jj, g->p, g->u, g->part_c, (const PgPcgState*)nullptr);
    if (hipEventRecord(e0, g->st) != hipSuccess) rc = fail(STBA_ERR_HIP, "hipEventRecord");
    for (int k = 0; k < reps && rc == STBA_OK; ++k) rc = pg_linearize(g, g->cur, true);
    if (rc == STBA_OK && hipEventRecord(e1, g->st) != hipSuccess) rc = fail(STBA_ERR_HIP, "hipEventRecord");
    for (int k = 0; k < reps && rc == STBA_OK; ++k)
        hipLaunchKernelGGL(pg_edge_product_kernel, dim3(g->nb_edges), dim3(256), 0, g->st, g->m, g->ei, g->ej, g->Ji, g->Jj, g->p, g->u, g->part_c, (const PgPcgState*)nullptr);
    if (rc == STBA_OK && hipEventRecord(e2, g->st) != hipSuccess) rc = fail(STBA_ERR_HIP, "hipEventRecord");
    if (rc == STBA_OK && hipStreamSynchronize(g->st) != hipSuccess) rc = fail(STBA_ERR_HIP, "hipStreamSynchronize");
    float a = 0.f, b = 0.f;
    if (rc == STBA_OK) { (void)hipEventElapsedTime(&a, e0, e1); (void)hipEventElapsedTime(&b, e1, e2); }
    (void)hipEventDestroy(e0); (void)hipEventDestroy(e1); (void)hipEventDestroy(e2);
    *ms_linearize = a / reps; *ms_matvec = b / reps;
    return rc;
}

int stba_pg_solve(stba_pg* g, const stba_lm_options* opt_in, const stba_pcg_options* pcg_in, stba_lm_summary* summary,
                  double* trace, int* pcg_iterations_total) {
    if (!g) return fail(STBA_ERR_INVALID_ARGUMENT, "null engine");
    stba_lm_options opt;
    if (opt_in) opt = *opt_in; else stba_lm_default_options(&opt);
    stba_pcg_options pcg;
    if (pcg_in) pcg = *pcg_in; else stba_pcg_default_options(&pcg);
    stba_lm_summary s;
    memset(&s, 0, sizeof s);
    const double t0 = wall_s();
    // ---- options and set-up
    PgSolve sv(opt, pcg);
    STBA_TRY(pg_solve_begin(g, sv));
    stba_pcg_summary& ps = sv.ps;
    TrustRegion& region = sv.region;
    const double* fin = g->fin_vals;          // (the validated copy of the mapped block g->fin)

    // ---- first linearisation
    STBA_TRY(pg_linearize_enqueue(g, sv));
    STBA_TRY(pg_linearize_finish(g, &sv.cost, &sv.gmax, &sv.g2));
    s.initial_cost = sv.cost;
    trace_start(trace, sv.cost, sv.gmax, region.radius);
    s.termination_type = STBA_NO_CONVERGENCE; s.termination_reason = STBA_TERM_MAX_ITER;
    bool done = sv.gmax <= opt.gradient_tolerance;
    if (done) { s.termination_type = STBA_CONVERGENCE; s.termination_reason = STBA_TERM_GRADIENT; }
    if (!std::isfinite(sv.cost)) { s.termination_type = STBA_FAILURE; s.termination_reason = STBA_TERM_SOLVER_FAIL; done = true; }   // (Ceres: initial evaluation failed, see stba_ba_solve)
    while (!done) {
        if (sv.iter >= opt.max_num_iterations) break;
        if (region.below_min(opt)) { s.termination_type = STBA_CONVERGENCE; s.termination_reason = STBA_TERM_MIN_RADIUS; break; }
        ++sv.iter;
        // ---- preconditioner (behind an accepted step it and the job's head are already on their way)
        const bool head_was_done = sv.head_done;
        if (!sv.head_done) {
            STBA_TRY(pg_wait_for_job_reads(g));      // (a rejected step: no linearisation in between)
            pg_precond(g, sv);
        }
        sv.head_done = false;
        PgCoarseUse cu;
        STBA_TRY(pg_coarse_refresh(g, sv, head_was_done, &cu));
        // ---- PCG and trial point.  A deferred job goes BEHIND the launch of the one-kernel PCG, so that the host enqueues it while
        // the kernel runs, but in FRONT of the launch path's, which talks to the host all along (pg_job_rest: the measured reason)
        const double eta_k = sv.forcing ? sv.eta : pcg.relative_tolerance;
        const int nxt = g->cur ^ 1;
        const bool one_kernel = sv.pp_ok && !g->pp_disabled;
        if (sv.timing && !g->ev_t[0]) { STBA_HIP(hipEventCreate(&g->ev_t[0])); STBA_HIP(hipEventCreate(&g->ev_t[1])); }
        if (sv.timing) STBA_HIP(hipEventRecord(g->ev_t[0], g->st));
        if (!one_kernel && cu.job_deferred) { STBA_TRY(pg_job_rest(g, sv, cu.job)); cu.job_deferred = false; }
        if (one_kernel) STBA_TRY(pg_pcg_one_kernel(g, sv, cu.Ainv, eta_k)); else STBA_TRY(pg_pcg_by_launches(g, sv, cu.Ainv, eta_k));
        if (sv.timing) STBA_HIP(hipEventRecord(g->ev_t[1], g->st));
        if (cu.job_deferred) { STBA_TRY(pg_job_rest(g, sv, cu.job)); cu.job_deferred = false; }
        STBA_TRY(pg_trial_point(g));
        if (sv.timing) {
            float ms = 0.f;
            STBA_HIP(hipEventSynchronize(g->ev_t[1]));
            STBA_HIP(hipEventElapsedTime(&ms, g->ev_t[0], g->ev_t[1]));
            ps.linear_solve_ms += (double)ms;
        }
        if (one_kernel && fin[6] != (double)PP_TIMED_OUT) ++ps.one_kernel_solves;
        if (one_kernel && fin[6] == (double)PP_TIMED_OUT) {
            // a stamp never came: the workgroups were not all resident (another process on the device).  Once is enough: this
            // engine solves with launches from here on, starting with this very iteration.
            g->pp_disabled = true;
            STBA_TRY(pg_pcg_by_launches(g, sv, cu.Ainv, eta_k));
            STBA_TRY(pg_trial_point(g));
        }
        // ---- verdict
        const double new_cost = 0.5 * fin[0], xhx = fin[1], gx = fin[2], step2 = fin[3], x2 = fin[4];
        const int k = (int)fin[5];
        const bool capped = fin[6] != 0.0;
        const double rr0 = fin[7];
        ps.iterations_total += k; ++ps.solves; ps.hit_cap += capped ? 1 : 0; ps.max_iterations_in_a_solve = std::max(ps.max_iterations_in_a_solve, k);
        ps.last_eta = eta_k;
        bool ok = std::isfinite(rr0);
        const double model_change = -gx - 0.5 * xhx;
        const double step_norm = std::sqrt(step2), x_norm = std::sqrt(x2);
        ok = ok && model_change > 0.0 && std::isfinite(model_change) && std::isfinite(new_cost);
        const StepVerdict v = judge_step(opt, sv.cost, ok, new_cost, model_change, step_norm, x_norm);
        trace_step(trace, sv.iter, ok, sv.cost, new_cost, v, sv.gmax, step_norm, region.radius);
        if (v.stop) {        // (no progress line)
            s.termination_type = STBA_CONVERGENCE; s.termination_reason = v.stop;
            if (v.accepted) { g->cur = nxt; sv.cost = new_cost; ++s.num_successful_steps; g->coarse_valid = false; }
            break;
        }
        if (v.accepted) {
            g->cur = nxt;
            ++s.num_successful_steps;
            sv.last_rel_decrease = sv.cost > 0.0 ? v.cost_change / sv.cost : 1.0;
            region.accept(v.rho, opt);
            double g2_new = 0.0;
            STBA_TRY(pg_linearize_enqueue(g, sv));
            if (sv.async_inv && sv.build_on_st2) {        // the next iteration's preconditioner kernel and the head of its job, at once (pg_job_head)
                pg_precond(g, sv);
                STBA_HIP(hipEventRecord(g->ev_in, g->st));
                STBA_TRY(pg_job_head(g));
                sv.head_done = true;
            }
            STBA_TRY(pg_linearize_finish(g, &sv.cost, &sv.gmax, &g2_new));
            sv.eta = pg_next_eta(pcg, opt, sv.eta, sv.g2, g2_new, v.cost_change, sv.cost);
            sv.g2 = g2_new;
            if (trace) { trace[(size_t)sv.iter * STBA_TRACE_COLS + 2] = sv.gmax; trace[(size_t)sv.iter * STBA_TRACE_COLS + 5] = region.radius; }
            // (the gradient is tested here, before the progress line: none is printed for the converging iteration)
            if (sv.gmax <= opt.gradient_tolerance) { s.termination_type = STBA_CONVERGENCE; s.termination_reason = STBA_TERM_GRADIENT; break; }
        } else {
            ++s.num_unsuccessful_steps;
            region.reject();
            if (trace) trace[(size_t)sv.iter * STBA_TRACE_COLS + 5] = region.radius;
        }
        if (opt.minimizer_progress_to_stdout) {
            char tail[64];
            snprintf(tail, sizeof tail, "  pcg %d eta %.1e%s", k, eta_k, capped ? " CAP" : "");
            progress_step(sv.iter, sv.cost, v, sv.gmax, step_norm, region.radius, tail);
        }
    }
    // ---- summary
    finish_summary(&s, sv.iter, sv.cost, region.radius, sv.gmax, t0);
    if (summary) *summary = s;
    if (pcg_iterations_total) *pcg_iterations_total = ps.iterations_total;
    if (sv.coarse) {        // (how many coarse operators could not be factored: counted on the device, read once per solve)
        int cf = 0;
        if (hipMemcpyAsync(&cf, g->cflag + 1, sizeof(int), hipMemcpyDeviceToHost, g->st) == hipSuccess && hipStreamSynchronize(g->st) == hipSuccess)
            ps.coarse_failures = cf;
    }
    g->last_pcg = ps;
    return STBA_OK;
}

// the two setters of the per-edge weights: `in` [m][36] -> a NEW component-major array on the device; only a call that succeeds
// swaps it in (a refused one leaves the engine with the weights it had), NULL releases the array
static int pg_set_weights(stba_pg* g, const double* in, int sqrt_form, const char* who) {
    if (!g) return fail(STBA_ERR_INVALID_ARGUMENT, std::string(who) + ": null engine");
    DevBuf<double> Wnew;
    if (in) {
        const size_t cnt = (size_t)g->m * 36;
        DevBuf<double> stage;
        DevBuf<int> bad;
        int bad_h = INT_MAX;
        STBA_TRY(Wnew.alloc(cnt)); STBA_TRY(stage.alloc(cnt)); STBA_TRY(bad.alloc(1));
        if (upload(stage, in, cnt, g->st) != STBA_OK || upload(bad, &bad_h, 1, g->st) != STBA_OK)
            return fail(STBA_ERR_HIP, std::string(who) + ": upload failed");
        hipLaunchKernelGGL(pg_information_kernel, dim3(g->nb_edges), dim3(256), 0, g->st, g->m, (const double*)stage, sqrt_form, Wnew.get(), bad.get());
        if (hipGetLastError() != hipSuccess || download(&bad_h, bad, 1, g->st) != STBA_OK || hipStreamSynchronize(g->st) != hipSuccess)
            return fail(STBA_ERR_HIP, std::string(who) + ": the conversion kernel failed");
        if (bad_h != INT_MAX)
            return sqrt_form ? fail(STBA_ERR_INVALID_ARGUMENT, std::string(who) + ": edge " + std::to_string(bad_h) + ": the square-root information has an entry that is not finite")
                             : fail(STBA_ERR_NOT_POSITIVE_DEFINITE, std::string(who) + ": edge " + std::to_string(bad_h) + ": the information matrix is not positive definite (or has an entry that is not finite)");
    }
    // (nothing of the engine may still be reading the old array or what was linearised with it: the move below frees it)
    STBA_HIP(hipStreamSynchronize(g->st));
    if (g->st2) { STBA_HIP(hipStreamSynchronize(g->st2)); g->job_in_flight = false; g->job_reads_pending = false; }
    g->Winfo = std::move(Wnew);
    g->bend_valid = false; g->coarse_valid = false; g->ac0_valid = false;      // what pg_linearize and the solve's linearisation reset
    return STBA_OK;
}

int stba_pg_set_information(stba_pg* g, const double* information) { return pg_set_weights(g, information, 0, "stba_pg_set_information"); }
int stba_pg_set_sqrt_information(stba_pg* g, const double* sqrt_information) { return pg_set_weights(g, sqrt_information, 1, "stba_pg_set_sqrt_information"); }
int stba_pg_has_information(const stba_pg* g, int* has) {
    if (!g || !has) return fail(STBA_ERR_INVALID_ARGUMENT, "null argument");
    *has = g->Winfo ? 1 : 0;
    return STBA_OK;
}

// the per-edge loss table: checked on the host BEFORE anything is replaced (a refused call leaves the engine with the table it had),
// then uploaded into NEW arrays that are swapped in; kind == NULL releases the table
int stba_pg_set_loss(stba_pg* g, const int* kind, const double* a, const double* b, const double* scale) {
    const char* who = "stba_pg_set_loss";
    if (!g) return fail(STBA_ERR_INVALID_ARGUMENT, std::string(who) + ": null engine");
    DevBuf<int> k_new;
    DevBuf<double> a_new, b_new, s_new;
    if (kind) {
        const size_t m = (size_t)g->m;
        std::vector<double> ha, hb, hs;
        STBA_TRY(loss_table_check(who, "edge", m, kind, a, b, scale, ha, hb, hs));
        STBA_TRY(k_new.alloc(m)); STBA_TRY(a_new.alloc(m)); STBA_TRY(b_new.alloc(m)); STBA_TRY(s_new.alloc(m));
        if (upload(k_new, kind, m, g->st) != STBA_OK || upload(a_new, ha.data(), m, g->st) != STBA_OK ||
            upload(b_new, hb.data(), m, g->st) != STBA_OK || upload(s_new, hs.data(), m, g->st) != STBA_OK ||
            hipStreamSynchronize(g->st) != hipSuccess)
            return fail(STBA_ERR_HIP, std::string(who) + ": upload failed");
    }
    // (nothing of the engine may still be reading the old table or what was linearised with it: the moves below free it)
    STBA_HIP(hipStreamSynchronize(g->st));
    if (g->st2) { STBA_HIP(hipStreamSynchronize(g->st2)); g->job_in_flight = false; g->job_reads_pending = false; }
    g->loss_kind = std::move(k_new); g->loss_a = std::move(a_new); g->loss_b = std::move(b_new); g->loss_scale = std::move(s_new);
    g->bend_valid = false; g->coarse_valid = false; g->ac0_valid = false;
    return STBA_OK;
}

int stba_pg_has_loss(const stba_pg* g, int* has) {
    if (!g || !has) return fail(STBA_ERR_INVALID_ARGUMENT, "null argument");
    *has = g->loss_kind ? 1 : 0;
    return STBA_OK;
}

int stba_pg_last_pcg_summary(stba_pg* g, stba_pcg_summary* out) {
    if (!g || !out) return fail(STBA_ERR_INVALID_ARGUMENT, "null argument");
    *out = g->last_pcg;
    return STBA_OK;
}

}  // extern "C"
