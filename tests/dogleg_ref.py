"""An independent dense reference of Powell's dogleg (Ceres' TrustRegionMinimizer + DoglegStrategy, TRADITIONAL_DOGLEG) for the
bundle adjustment, written from the rules of DESIGN.md 7c, not from the engine.  CPU only.  It reuses lm_step_ref's problems, its
long-double normal equations and its refined dense solve: no Schur complement, nothing shared with the device.

Rules, as restated here:
  d_i      = sqrt(clamp(s_i^2 H_ii, min_lm_diagonal, max_lm_diagonal)), s the Jacobi scale fixed at iteration 0
  gamma    = (s .* g) ./ d;  alpha = |gamma|^2 / |J (s .* gamma ./ d)|^2
  y_gn     solves (S H S + mu diag(d^2)) y = -S g over the free unknowns; mu starts at 1e-8, x10 while the Cholesky fails or the step
           is not finite (mu < 1), else the step is invalid;  z_gn = d .* y_gn
  step     in z = d .* y:  |z_gn| <= Delta: z_gn;  alpha |gamma| >= Delta: -(Delta / |gamma|) gamma;  else the point at distance Delta
           of the segment from -alpha gamma to z_gn;  delta = s .* (z ./ d), applied with the problem's plus
  model    m = -(J delta)^T (r + J delta / 2), formed from J and r (not from the six scalars the engine uses)
  accepted Delta *= 0.5 if rho < 0.25, Delta = max(Delta, 3 |z|) if rho > 0.75, capped; mu = max(1e-8, mu / 5); new linearisation
  rejected Delta *= 0.5, the next step re-uses gamma, alpha and z_gn
  invalid  (no GN step, or m <= 0 / not finite): mu *= 10, no re-use
Each deliberate mistake of MUTATIONS turns one rule into a plausible wrong one; test_dogleg_reference.py shows that each moves a
trace row by more than the GPU tests' bound."""
import numpy as np

import lm_step_ref as L

LD = L.LD
MIN_MU, MAX_MU, MU_INCREASE = 1e-8, 1.0, 10.0
MUTATIONS = ("radius_in_y", "alpha_without_d", "other_beta_root", "mu_never_decreased", "mu_zero")
CASES = ("gauss_newton", "cauchy", "interpolated")


def traditional_dogleg(cauchy, gn, radius, mut=()):
    """the dogleg point of the path 0 -> cauchy -> gn at distance radius: (point, case index, beta)"""
    gn_norm, c_norm = np.linalg.norm(gn), np.linalg.norm(cauchy)
    if gn_norm <= radius:
        return gn.copy(), 0, 1.0
    if c_norm >= radius:
        return (radius / c_norm) * cauchy, 1, 0.0
    a, b = cauchy.astype(LD), gn.astype(LD)
    ba = float(b @ a)
    a2 = float(a @ a)
    bma2 = float((b - a) @ (b - a))
    c = ba - a2
    q = np.sqrt(c * c + bma2 * (radius * radius - a2))
    if "other_beta_root" in mut:
        beta = (-c - q) / bma2
    else:
        beta = (q - c) / bma2 if c <= 0 else (radius * radius - a2) / (q + c)
    return (1.0 - beta) * cauchy + beta * gn, 2, float(beta)


def dogleg_reference(prob, opt, k, mut=frozenset()):
    """k iterations from prob.x0; per iteration the keys of lm_step_ref.lm_reference plus case, beta, mu (after the iteration),
    z_norm, reused, escalations (mu raises inside the iteration), valid; out[0]['start'] holds the start point's cost / gmax / radius"""
    mut = frozenset(mut)
    n = prob.n_local
    fidx = np.nonzero(prob.free)[0]
    x = prob.x0.copy()
    radius = float(opt["initial_trust_region_radius"])
    mu = 0.0 if "mu_zero" in mut else MIN_MU
    dmin, dmax = opt["min_lm_diagonal"], opt["max_lm_diagonal"]

    def linearise(x):
        r, J, cols = prob.lin(x, True)
        H, g = L.normal_equations(n, r, J, cols)
        return r, J, cols, H, g

    def jdot(J, cols, v):
        return np.einsum("bea,ba->be", J.astype(LD), v.astype(LD)[cols])

    def gmax_of(g):
        return float(np.abs(g.astype(np.float64)[fidx]).max()) if len(fidx) else 0.0

    r, J, cols, H, g = linearise(x)
    cost = float(0.5 * np.sum(r.astype(LD) ** 2))
    start = dict(cost=cost, gmax=gmax_of(g), radius=radius)
    s = None
    lin = None           # what a rejected step re-uses
    out = []
    for it in range(k):
        reused = lin is not None
        escalations = 0
        if lin is None:
            Hd = np.diag(H).astype(np.float64)
            if s is None:
                s = 1.0 / (1.0 + np.sqrt(Hd)) if opt["jacobi_scaling"] else np.ones(n)
            d2 = np.clip(s * s * Hd, dmin, dmax)
            d = np.sqrt(d2)[fidx]
            sL = s.astype(LD)
            A0 = (H * sL[:, None] * sL[None, :])[np.ix_(fidx, fidx)]
            gh = (sL * g)[fidx]
            gamma = (gh / d).astype(np.float64)
            u = gamma if "alpha_without_d" in mut else gamma / d
            du = np.zeros(n); du[fidx] = s[fidx] * u
            ju = jdot(J, cols, du)
            alpha = float(np.sum(gamma.astype(LD) ** 2) / np.sum(ju * ju))
            y_gn, A = None, None
            while True:
                if "mu_zero" not in mut and not mu < MAX_MU:
                    break
                A = A0 + np.diag((mu * d * d).astype(LD))
                try:
                    np.linalg.cholesky(A.astype(np.float64))
                    y = L.refined_solve(A, -gh).astype(np.float64)
                    ok = np.all(np.isfinite(y))
                except np.linalg.LinAlgError:
                    ok = False
                if ok:
                    y_gn = y
                    break
                if "mu_zero" in mut:
                    break
                mu *= MU_INCREASE
                escalations += 1
            lin = None if y_gn is None else dict(gamma=gamma, alpha=alpha, y_gn=y_gn, z_gn=d * y_gn, d=d,
                                                  kappa=L.kappa2(A))
        valid = lin is not None
        if valid:
            gamma, alpha, d = lin["gamma"], lin["alpha"], lin["d"]
            if "radius_in_y" in mut:
                y, kase, beta = traditional_dogleg(-alpha * gamma / d, lin["y_gn"], radius, mut)
                z = d * y
            else:
                z, kase, beta = traditional_dogleg(-alpha * gamma, lin["z_gn"], radius, mut)
                y = z / d
            delta = np.zeros(n)
            delta[fidx] = s[fidx] * y
            f = jdot(J, cols, delta)
            model = float(-np.sum(f * (r.astype(LD) + f / 2)))
            valid = np.isfinite(model) and model > 0.0
            kappa = lin["kappa"]
        else:
            z, kase, beta, delta, model, kappa = np.zeros(len(fidx)), -1, 0.0, np.zeros(n), np.float64(0.0), 1.0
        xt = prob.plus(x, delta)
        trial_cost = prob.cost(xt) if valid else cost
        ok = valid and np.isfinite(trial_cost)
        step_norm = float(np.linalg.norm(xt - x)) if ok else 0.0
        x_norm = float(np.linalg.norm(x[prob.x_norm_mask]))
        cost_change = cost - trial_cost if ok else 0.0
        rho = cost_change / model if ok else 0.0
        accepted = bool(ok and rho > opt["min_relative_decrease"])
        radius_before = radius
        z_norm = float(np.linalg.norm(z))
        if accepted:
            if rho > 0.75:
                radius = max(radius, 3.0 * z_norm)
            elif rho < 0.25:
                radius *= 0.5
            radius = min(opt["max_trust_region_radius"], radius)
            if "mu_never_decreased" not in mut and "mu_zero" not in mut:
                mu = max(MIN_MU, 2.0 * mu / MU_INCREASE)
            x, cost = xt, trial_cost
            r, J, cols, H, g = linearise(x)
            lin = None
        elif not valid:
            if "mu_zero" not in mut:
                mu *= MU_INCREASE
            lin = None
        else:
            radius *= 0.5
        out.append(dict(delta=delta, x=x.copy(), x_trial=xt, cost=cost, trial_cost=trial_cost if ok else cost,
                        cost_change=cost_change, model_change=model, rho=rho, step_norm=step_norm, x_norm=x_norm, gmax=gmax_of(g),
                        radius=radius, radius_before=radius_before, accepted=accepted, kappa=kappa, start=start, case=kase,
                        beta=beta, z=z, z_norm=z_norm, mu=mu, reused=reused, escalations=escalations, valid=bool(valid)))
    return out


def trace_rows(ref):
    return L.trace_rows(ref)


def radius_exact(it):
    """the radius rule of this step has no continuous input (halved, kept or capped): the device's must be bitwise the reference's
    ratio; False where it grew to 3 |z|"""
    return not (it["accepted"] and it["rho"] > 0.75 and 3.0 * it["z_norm"] > it["radius_before"])


def compare(prob, ref, opt, x_dev, trace_dev, path="ba"):
    """the device's end point and trace rows 1..k against the reference, with lm_step_ref's C * kappa * eps bounds for every column
    except the radius, which is checked here: a ratio of the device's own previous radius where the rule has no continuous input,
    else within the bound of |z| (u * radius).  Returns (failures, ratios) as lm_step_ref.compare does."""
    tol = L.tolerances(ref, path, opt)
    fails, ratios = [], {}
    kap = tol[-1]["kappa"]

    def note(name, err, bound, scale):
        ratios[name] = max(ratios.get(name, 0.0), err / max(kap * L.EPS * scale, 1e-300))
        if not err <= bound:
            fails.append(f"{name}: err {err:.3e} > bound {bound:.3e}")

    ex = L.point_error(prob, x_dev, ref[-1]["x"])
    dsum = sum(np.linalg.norm(it["delta"]) for it in ref)
    xs = np.linalg.norm(ref[-1]["x"])
    note("point", ex, tol[-1]["u"] * dsum + L.C_PATH[path] * L.EPS * xs, dsum + xs / kap)
    rows = trace_rows(ref)
    for i in range(len(ref)):
        dv, rr, t, it = trace_dev[i + 1], rows[i], tol[i], ref[i]
        if dv[6] != rr[6]:
            fails.append(f"iteration {i + 1}: accepted {dv[6]} != reference {rr[6]}")
            continue
        note("cost", abs(dv[0] - rr[0]), t["cost"], rr[0])
        note("cost_change", abs(dv[1] - rr[1]), t["cost_change"], abs(rr[1]))
        note("gradient_max_norm", abs(dv[2] - rr[2]), t["gmax"], rr[2])
        note("step_norm", abs(dv[3] - rr[3]), t["step_norm"], rr[3])
        note("rho", abs(dv[4] - rr[4]), t["rho"], abs(rr[4]))
        if radius_exact(it):
            ratio = it["radius"] / it["radius_before"]
            expect = min(opt["max_trust_region_radius"], trace_dev[i][5] * ratio)
            if dv[5] != expect and not (ratio not in (0.5, 1.0) and abs(dv[5] - expect) <= 4 * L.EPS * expect):
                fails.append(f"iteration {i + 1}: radius {dv[5]!r} != {expect!r}")
        else:
            note("radius", abs(dv[5] - rr[5]), t["u"] * rr[5], rr[5])
    return fails, ratios


def decisions(ref):
    """per iteration (accepted, case, escalations): what a decisions-only comparison holds the device to"""
    return [(it["accepted"], it["case"], it["escalations"]) for it in ref]
