"""An independent numpy reference of the BA engine's inner iterations (Ceres' Solver::Options::use_inner_iterations), written from
the contract of DESIGN.md 7d -- Ceres' TrustRegionMinimizer::DoInnerIterationsIfNeeded / IsStepSuccessful and
CoordinateDescentMinimizer -- not from the device code.  CPU only.

  block LM   every block of a group solved on its own by a TrustRegionMinimizer with DEFAULT Solver::Options (LM, 50 iterations,
             function / gradient / parameter tolerance 1e-6 / 1e-10 / 1e-8, radius 1e4, max radius 1e32, Jacobi scaling at the block's
             start point); the function-tolerance step is NOT taken; the damped system is solved densely in np.longdouble sums
             (lm_step_ref.normal_equations, refined_solve) over the block's active dofs
  sweep      the groups in ascending id; a camera part is its rotation (dofs 0..2, q <- q (x) exp(dtheta)) and / or its position
             (dofs 3..5, t <- t + dt); constant parts ignored
  outer loop after every valid step: model change += cost(x+) - cost(x*), useful = cost(x*) < cost(x), the step is accepted if
             useful or rho > min_relative_decrease, step norm |x - x*| (ambient), sweeps stop once 1 - cost(x*) / cost(x+) <= tol

Residuals and Jacobians are lm_step_ref's BAProblem formulas (quat_to_rot on the quaternion as stored, hat, quat_exp, quat_mul).
Each deliberate mistake of MUTATIONS turns one rule into a plausible wrong one; test_inner_iterations_cpu.py shows that every
one of them moves a result on the test scenes by far more than the GPU tests' tolerance."""
import numpy as np

import lm_step_ref as R

LD = np.longdouble
EPS = np.finfo(np.float64).eps

MUTATIONS = ("no_model_adjust", "accept_rho_only", "never_switch_off", "groups_reversed", "caller_options_in_block",
             "block_ftol_takes_step", "step_norm_without_sweep")

BLOCK_OPTIONS = dict(max_num_iterations=50, function_tolerance=1e-6, gradient_tolerance=1e-10, parameter_tolerance=1e-8,
                     initial_trust_region_radius=1e4, max_trust_region_radius=1e32, min_trust_region_radius=1e-32,
                     min_relative_decrease=1e-3, min_lm_diagonal=1e-6, max_lm_diagonal=1e32)


def _obs(prob, cams, pts, idx, jac=True):
    """r [m, 2], Jc [m, 2, 6], Jp [m, 2, 3] of the observations idx (BAProblem.lin_obs, restricted)"""
    oc, op = prob.oc[idx], prob.op[idx]
    Rm = R.quat_to_rot(cams[oc, :4], normalise=False)
    p = np.einsum("nji,nj->ni", Rm, pts[op] - cams[oc, 4:])
    r = p[:, :2] / p[:, 2:3] - prob.f[idx]
    if not jac:
        return r, None, None
    z = p[:, 2]
    A = np.zeros((len(z), 2, 3))
    A[:, 0, 0] = A[:, 1, 1] = 1 / z; A[:, 0, 2] = -p[:, 0] / z ** 2; A[:, 1, 2] = -p[:, 1] / z ** 2
    Jp = A @ np.swapaxes(Rm, 1, 2)
    return r, np.concatenate([A @ R.hat(p), -Jp], 2), Jp


def _cost(r):
    return float(0.5 * np.sum(r.astype(LD) ** 2))


def block_lm(lin, cost_at, plus, x, active, norm_sel, opts=BLOCK_OPTIONS, ftol_takes_step=False):
    """Ceres' TrustRegionMinimizer (LM) on one block.  lin(x) -> (cost, H [n, n] LD, g [n] LD); cost_at(x); plus(x, d) -> x;
    active: bool [n]; norm_sel: ambient entries of |x| and |x - x+|.  Returns (x, iterations, stop)"""
    n = len(active)
    aidx = np.nonzero(active)[0]
    cost, H, g = lin(x)
    if not np.isfinite(cost):
        return x, 0, "invalid"
    Hd = np.diag(H).astype(np.float64)
    s = 1.0 / (1.0 + np.sqrt(Hd))
    gmax = lambda g: float(np.abs(g[aidx].astype(np.float64)).max())
    if gmax(g) <= opts["gradient_tolerance"]:
        return x, 0, "gradient"
    radius, v, it, invalid = float(opts["initial_trust_region_radius"]), 2.0, 0, 0
    while True:
        if it >= opts["max_num_iterations"]:
            return x, it, "max_iter"
        if radius < opts["min_trust_region_radius"]:
            return x, it, "min_radius"
        it += 1
        Hd = np.diag(H).astype(np.float64)
        D = np.clip(s * s * Hd, opts["min_lm_diagonal"], opts["max_lm_diagonal"]) / radius
        sL = s.astype(LD)
        A = (H * sL[:, None] * sL[None, :])[np.ix_(aidx, aidx)] + np.diag(D[aidx].astype(LD))
        b = -(sL * g)[aidx]
        valid = True
        try:
            np.linalg.cholesky(np.asarray(A, dtype=np.float64))     # (a pivot that is not positive: the factorisation fails)
            y = R.refined_solve(A, b)
            d = np.zeros(n)
            d[aidx] = (sL[aidx] * y).astype(np.float64)
            dL = d.astype(LD)
            model = float(-(g @ dL + 0.5 * dL @ (H @ dL)))
            valid = np.isfinite(model) and model > 0.0
        except np.linalg.LinAlgError:
            valid = False
        if not valid:
            invalid += 1
            if invalid > 5:
                return x, it, "invalid"
            radius /= v; v *= 2.0
            continue
        invalid = 0
        xn = plus(x, d)
        new_cost = cost_at(xn)
        if not np.isfinite(new_cost):
            new_cost = np.inf
        if np.linalg.norm((x - xn)[norm_sel]) <= opts["parameter_tolerance"] * (np.linalg.norm(x[norm_sel]) + opts["parameter_tolerance"]):
            return x, it, "parameter"
        change = cost - new_cost
        if abs(change) <= opts["function_tolerance"] * cost:
            if ftol_takes_step and change / model > opts["min_relative_decrease"]:
                x = xn
            return x, it, "function"
        rho = change / model
        if rho > opts["min_relative_decrease"]:
            x = xn
            cost, H, g = lin(x)
            t = 2.0 * rho - 1.0
            radius = min(opts["max_trust_region_radius"], radius / max(1.0 / 3.0, 1.0 - t ** 3))
            v = 2.0
            if gmax(g) <= opts["gradient_tolerance"]:
                return x, it, "gradient"
        else:
            radius /= v; v *= 2.0


ORDERING_MUTATIONS = ("no_constant_masking", "groups_reversed", "no_independence_check")


def ordering(prob, rot=None, pos=None, pt=None, mut=frozenset()):
    """the C ABI's ordering (include/stba.h stba_ba_set_inner_iterations): list of (group id, [(camera, kind)], [landmarks]) in
    ascending id; kind 1 rotation, 2 position, 3 both.  All None: {cameras as 6-dof blocks}, {landmarks}.  Constant parts ignored.
    mut: deliberate mistakes of ORDERING_MUTATIONS (test_inner_plan_cpu.py shows that its cases tell each of them apart)"""
    nc, npt = prob.nc, prob.np_
    if rot is None and pos is None and pt is None:
        rot, pos, pt = np.zeros(nc, int), np.zeros(nc, int), np.ones(npt, int)
    rot = -np.ones(nc, int) if rot is None else np.asarray(rot, int)
    pos = -np.ones(nc, int) if pos is None else np.asarray(pos, int)
    pt = -np.ones(npt, int) if pt is None else np.asarray(pt, int)
    if "no_constant_masking" not in mut:
        rot = np.where(prob.rot_active, rot, -1)
        pos = np.where(prob.pos_active, pos, -1)
        pt = np.where(prob.pt_fixed, -1, pt)
    for c, j in zip(prob.oc, prob.op):
        if pt[j] >= 0 and pt[j] in (rot[c], pos[c]) and "no_independence_check" not in mut:
            raise ValueError(f"group {pt[j]} is not an independent set: camera {c} and landmark {j}")
    ids = sorted(set(rot[rot >= 0]) | set(pos[pos >= 0]) | set(pt[pt >= 0]), reverse="groups_reversed" in mut)
    out = []
    for gid in ids:
        cams = [(c, (1 if rot[c] == gid else 0) | (2 if pos[c] == gid else 0)) for c in range(nc) if gid in (rot[c], pos[c])]
        out.append((gid, cams, [j for j in range(npt) if pt[j] == gid]))
    return out


def ordering_lists(prob, rot=None, pos=None, pt=None, mut=frozenset()):
    """ordering() flattened into the five arrays of slam-tricks_amd/csrc/inner_plan.hpp: groups [(cam_lo, cam_hi, pt_lo, pt_hi)], the
    camera list, the landmark list, and per camera entry the swept dofs as a bit mask (sweep()'s rule: the kind's dofs that are not
    constant) and the kind"""
    groups, cam, pts, mask, kind = [], [], [], [], []
    for _, gcams, gpts in ordering(prob, rot, pos, pt, mut):
        lo = (len(cam), len(pts))
        for c, k in gcams:
            active = np.zeros(6, bool)
            if k & 1: active[:3] = True
            if k & 2: active[3:] = True
            if "no_constant_masking" not in mut:
                active &= ~prob.cam_fixed[c]
            cam.append(int(c)); kind.append(int(k)); mask.append(int(sum(1 << a for a in range(6) if active[a])))
        pts.extend(int(j) for j in gpts)
        groups.append((lo[0], len(cam), lo[1], len(pts)))
    return dict(groups=groups, cam=cam, pt=pts, mask=mask, kind=kind)


def sweep(prob, x, order, mut=frozenset(), opts=None):
    """one coordinate-descent sweep from x (flat, BAProblem layout).  Returns (x*, iterations {rot, pos, pt})"""
    mut = frozenset(mut)
    opts = opts or BLOCK_OPTIONS
    cams, pts = (a.copy() for a in prob.split(x.copy()))
    it = {"rot": np.zeros(prob.nc, int), "pos": np.zeros(prob.nc, int), "pt": np.zeros(prob.np_, int)}
    ftol_step = "block_ftol_takes_step" in mut
    groups = list(reversed(order)) if "groups_reversed" in mut else order
    for _, gcams, gpts in groups:
        new_cams = cams.copy()
        for c, kind in gcams:
            idx = np.nonzero(prob.oc == c)[0]
            if len(idx) == 0:
                continue
            active = np.zeros(6, bool)
            if kind & 1: active[:3] = True
            if kind & 2: active[3:] = True
            active &= ~prob.cam_fixed[c]
            if not active.any():
                continue
            rot_on, pos_on = bool(active[:3].any()), bool(active[3:].any())

            def lin(xc, idx=idx, c=c):
                cc = cams.copy(); cc[c] = xc
                r, Jc, _ = _obs(prob, cc, pts, idx)
                H, g = R.normal_equations(6, r, Jc, np.tile(np.arange(6), (len(idx), 1)))
                return _cost(r), H, g

            def cost_at(xc, idx=idx, c=c):
                cc = cams.copy(); cc[c] = xc
                return _cost(_obs(prob, cc, pts, idx, False)[0])

            def plus(xc, d, rot_on=rot_on, pos_on=pos_on):
                out = xc.copy()
                if rot_on:
                    q = R.quat_mul(xc[None, :4], R.quat_exp(d[None, :3]))[0]
                    out[:4] = q / np.linalg.norm(q)
                if pos_on:
                    out[4:] = xc[4:] + d[3:]
                return out

            sel = np.array([rot_on] * 4 + [pos_on] * 3)
            xc, n_it, _ = block_lm(lin, cost_at, plus, cams[c].copy(), active, sel, opts, ftol_step)
            new_cams[c] = xc
            if kind & 1: it["rot"][c] = n_it
            if kind & 2: it["pos"][c] = n_it
        new_pts = pts.copy()
        for j in gpts:
            idx = np.nonzero(prob.op == j)[0]
            if len(idx) == 0 or prob.pt_fixed[j]:
                continue

            def lin(L, idx=idx, j=j):
                pp = pts.copy(); pp[j] = L
                r, _, Jp = _obs(prob, cams, pp, idx)
                H, g = R.normal_equations(3, r, Jp, np.tile(np.arange(3), (len(idx), 1)))
                return _cost(r), H, g

            def cost_at(L, idx=idx, j=j):
                pp = pts.copy(); pp[j] = L
                return _cost(_obs(prob, cams, pp, idx, False)[0])

            L, n_it, _ = block_lm(lin, cost_at, lambda L, d: L + d, pts[j].copy(), np.ones(3, bool), np.ones(3, bool), opts, ftol_step)
            new_pts[j] = L
            it["pt"][j] = n_it
        cams, pts = new_cams, new_pts          # (a group is independent: its blocks saw the values from before the group)
    return np.concatenate([cams.reshape(-1), pts.reshape(-1)]), it


def outer_reference(prob, opt, k, order, tolerance=1e-3, mut=frozenset()):
    """k LM iterations (the engine's stba_ba_solve with its stop tests, lm_step_ref's dense step) with inner iterations.
    Returns (rows, start) with one dict per iteration: trial_cost (after the sweep), cost_change, model_change, rho, step_norm,
    radius, accepted, swept, useful, inner_on (after the iteration), stop; the loop ends at a stop like the engine's."""
    mut = frozenset(mut)
    n = prob.n_local
    free = prob.free
    fidx = np.nonzero(free)[0]
    x = prob.x0.copy()
    radius, v = float(opt["initial_trust_region_radius"]), 2.0
    takes = opt.get("function_tolerance_takes_step", 1)
    block_opts = dict(BLOCK_OPTIONS)
    if "caller_options_in_block" in mut:
        block_opts.update({kk: opt[kk] for kk in BLOCK_OPTIONS if kk in opt})

    def linearise(x):
        r, J, cols = prob.lin(x, True)
        H, g = R.normal_equations(n, r, J, cols)
        return r, J, cols, H, g

    r, J, cols, H, g = linearise(x)
    cost = _cost(r)
    gmax = float(np.abs(g[fidx].astype(np.float64)).max())
    start = dict(cost=cost, gmax=gmax, radius=radius)
    inner_on = True
    scale = 1.0 / (1.0 + np.sqrt(np.diag(H).astype(np.float64)))
    rows = []
    if gmax <= opt["gradient_tolerance"]:
        return rows, start
    for it in range(1, k + 1):
        if radius < opt["min_trust_region_radius"]:
            break
        s = scale
        D = np.clip(s * s * np.diag(H).astype(np.float64), opt["min_lm_diagonal"], opt["max_lm_diagonal"]) / radius
        sL = s.astype(LD)
        A = (H * sL[:, None] * sL[None, :])[np.ix_(fidx, fidx)] + np.diag(D[fidx].astype(LD))
        y = R.refined_solve(A, -(sL * g)[fidx])
        delta = np.zeros(n)
        delta[fidx] = (sL[fidx] * y).astype(np.float64)
        f = np.einsum("bea,ba->be", J.astype(LD), delta.astype(LD)[cols])
        model = float(-np.sum(f * (r.astype(LD) + f / 2)))
        xt = prob.plus(x, delta)
        trial_cost = prob.cost(xt)
        step_norm = float(np.linalg.norm(xt - x))
        x_norm = float(np.linalg.norm(x[prob.x_norm_mask]))
        ok = np.isfinite(model) and model > 0 and np.isfinite(trial_cost)
        swept = useful = False
        if ok and inner_on:
            xs, _ = sweep(prob, xt, order, mut, block_opts)
            inner_cost = prob.cost(xs)
            swept = True
            if "no_model_adjust" not in mut:
                model += trial_cost - inner_cost
            useful = inner_cost < cost
            progress = 1.0 - inner_cost / trial_cost
            xt, trial_cost = xs, inner_cost
            if "step_norm_without_sweep" not in mut:
                step_norm = float(np.linalg.norm(xt - x))
            if not progress > tolerance and "never_switch_off" not in mut:
                inner_on = False
        if "accept_rho_only" in mut:
            useful = False
        row = dict(trial_cost=trial_cost, cost_change=0.0, model_change=model, rho=0.0, step_norm=step_norm, swept=swept,
                   useful=useful, accepted=False, stop=None, x_trial=xt)
        if ok:
            change = cost - trial_cost
            rho = change / model
            row.update(cost_change=change, rho=rho)
            if step_norm <= opt["parameter_tolerance"] * (x_norm + opt["parameter_tolerance"]):
                row["stop"] = "parameter"
            elif abs(change) <= opt["function_tolerance"] * cost:
                row["stop"] = "function"
                row["accepted"] = bool(takes and (useful or rho > opt["min_relative_decrease"]))
            else:
                row["accepted"] = bool(useful or rho > opt["min_relative_decrease"])
        if row["accepted"]:
            x, cost = xt, trial_cost
            r, J, cols, H, g = linearise(x)
            gmax = float(np.abs(g[fidx].astype(np.float64)).max())
        if row["stop"] is None:
            if row["accepted"]:
                t3 = 2.0 * row["rho"] - 1.0
                radius = min(opt["max_trust_region_radius"], radius / max(1.0 / 3.0, 1.0 - t3 ** 3))
                v = 2.0
            else:
                radius /= v
                v *= 2.0
        row.update(radius=radius, inner_on=inner_on, gmax=gmax, x=x.copy(), cost=cost)
        rows.append(row)
        if row["stop"] is not None or (row["accepted"] and gmax <= opt["gradient_tolerance"]):
            break
    return rows, start


def trace_rows(rows):
    """the engine's trace rows 1..k (STBA_TRACE_COLS) of the reference; the gradient column is the post-iteration gmax"""
    return np.array([[r["trial_cost"], r["cost_change"], r["gmax"], r["step_norm"], r["rho"], r["radius"], 1.0 if r["accepted"] else 0.0]
                     for r in rows])
