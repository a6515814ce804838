"""The cases of tests/cpp/ceres_routes_driver.cpp: one Solve() or Covariance::Compute() each, on the driver's tiny problems
(3 cameras x 8 landmarks; a 5-node ring of poses; one bounded scalar).  A case is "name key=value ...": the keys are the
driver's (Build / MakeOptions / MakePairs); s_ cases call Solve, c_ cases (kind=cov) Covariance::Compute.  The goldens under tests/golden/ceres_routes_*.json hold what the header did with
each case before its routing was rewritten; test_ceres_routes_cpu.py and test_gpu_ceres_routes.py compare against them."""
import json
import os
import subprocess

from conftest import ROOT

FIELDS = ("term", "path", "kept", "evals", "callbacks", "iters", "cost", "extra", "message", "stderr")

CASES = """
s_builtin prob=builtin
s_builtin_iter_identity prob=builtin ls=iterative_schur pc=identity
s_builtin_iter_jacobi prob=builtin ls=iterative_schur pc=jacobi
s_builtin_iter_schur_jacobi prob=builtin ls=iterative_schur pc=schur_jacobi
s_builtin_iter_cluster_jacobi prob=builtin ls=iterative_schur pc=cluster_jacobi
s_builtin_iter_cluster_tridiagonal prob=builtin ls=iterative_schur pc=cluster_tridiagonal
s_builtin_iter_subset prob=builtin ls=iterative_schur pc=subset
s_user prob=user
s_user_iter_cluster_tridiagonal prob=user ls=iterative_schur pc=cluster_tridiagonal
s_user_iter_subset prob=user ls=iterative_schur pc=subset
s_scaled prob=scaled
s_scaled_iter_cluster_jacobi prob=scaled ls=iterative_schur pc=cluster_jacobi
s_scaled_iter_subset prob=scaled ls=iterative_schur pc=subset
s_moved prob=moved
s_moved_iter_jacobi prob=moved ls=iterative_schur pc=jacobi
s_mixed prob=mixed
s_pg prob=pg
s_bound prob=bound
s_builtin_dogleg prob=builtin tr=dogleg
s_user_dogleg prob=user tr=dogleg
s_scaled_dogleg prob=scaled tr=dogleg
s_moved_dogleg prob=moved tr=dogleg
s_pg_dogleg prob=pg tr=dogleg
s_builtin_subspace prob=builtin tr=subspace
s_builtin_dogleg_iter prob=builtin tr=dogleg ls=iterative_schur
s_builtin_dogleg_force prob=builtin tr=dogleg force=1
s_builtin_dogleg_prior prob=builtin tr=dogleg prior=1
s_user_dogleg_prior prob=user tr=dogleg prior=1
s_builtin_dogleg_rel prob=builtin tr=dogleg rel=1
s_builtin_dogleg_prior_rel prob=builtin tr=dogleg prior=1 rel=1
s_builtin_dogleg_otherchart prob=builtin tr=dogleg chart=other
s_builtin_inner_default prob=builtin inner=default
s_builtin_inner_ok prob=builtin inner=ok
s_builtin_inner_partial prob=builtin inner=partial
s_builtin_inner_dep_cam prob=builtin inner=dep_cam
s_builtin_inner_dep_pt prob=builtin inner=dep_pt
s_builtin_inner_foreign prob=builtin inner=foreign
s_user_inner_foreign prob=user inner=foreign
s_builtin_inner_negtol prob=builtin inner=negtol
s_scaled_inner_default prob=scaled inner=default
s_moved_inner_default prob=moved inner=default
s_pg_inner_default prob=pg inner=default
s_bound_inner_default prob=bound inner=default
s_builtin_inner_dogleg prob=builtin inner=default tr=dogleg
s_builtin_inner_force prob=builtin inner=default force=1
s_builtin_inner_weighted prob=builtin inner=default weighted=some
s_builtin_inner_prior prob=builtin inner=default prior=1
s_builtin_inner_rel prob=builtin inner=default rel=1
s_builtin_inner_otherchart prob=builtin inner=default chart=other
s_builtin_loss_huber prob=builtin loss=huber
s_builtin_loss_huber_optin prob=builtin loss=huber ba_losses=1
s_builtin_loss_unknown_optin prob=builtin loss=unknown ba_losses=1
s_user_loss_huber prob=user loss=huber
s_user_loss_huber_optin prob=user loss=huber ba_losses=1
s_scaled_loss_huber_optin prob=scaled loss=huber ba_losses=1
s_moved_loss_huber prob=moved loss=huber
s_moved_loss_huber_optin prob=moved loss=huber ba_losses=1
s_pg_loss_huber prob=pg loss=huber
s_pg_loss_unknown prob=pg loss=unknown
s_bound_loss_huber prob=bound loss=huber
s_builtin_loss_scaled_optin prob=builtin loss=scaled ba_losses=1 loss_on=some
s_pg_loss_scaled prob=pg loss=scaled loss_on=some
s_builtin_loss_scalednull_optin prob=builtin loss=scalednull ba_losses=1 loss_on=some
s_builtin_loss_scaledscaled_optin prob=builtin loss=scaledscaled ba_losses=1 loss_on=some
s_pg_loss_scaledscaled prob=pg loss=scaledscaled loss_on=some
s_builtin_loss_optin_force prob=builtin loss=huber ba_losses=1 force=1
s_builtin_loss_optin_inner prob=builtin loss=huber ba_losses=1 inner=default
s_builtin_loss_optin_dogleg prob=builtin loss=huber ba_losses=1 tr=dogleg
s_builtin_loss_optin_iter prob=builtin loss=huber ba_losses=1 ls=iterative_schur
s_builtin_loss_optin_iter_subset prob=builtin loss=huber ba_losses=1 ls=iterative_schur pc=subset
s_builtin_loss_optin_weighted prob=builtin loss=huber ba_losses=1 weighted=some loss_on=some
s_builtin_loss_optin_prior prob=builtin loss=huber ba_losses=1 prior=1 loss_on=some
s_pg_loss_force prob=pg loss=huber force=1
s_pg_loss_cb prob=pg loss=huber cb=count
s_builtin_prior prob=builtin prior=1
s_builtin_rel prob=builtin rel=1
s_user_prior prob=user prior=1
s_scaled_prior prob=scaled prior=1
s_moved_prior prob=moved prior=1
s_builtin_prior_rel prob=builtin prior=1 rel=1
s_builtin_prior_loss prob=builtin prior=loss
s_builtin_rel_loss_optin prob=builtin rel=loss ba_losses=1
s_builtin_prior_mismatch prob=builtin prior=mismatch
s_builtin_rel_same prob=builtin rel=same
s_builtin_prior_iter prob=builtin prior=1 ls=iterative_schur
s_builtin_rel_iter prob=builtin rel=1 ls=iterative_schur
s_builtin_prior_rel_iter prob=builtin prior=1 rel=1 ls=iterative_schur
s_builtin_prior_force prob=builtin prior=1 force=1
s_builtin_weighted_some prob=builtin weighted=some
s_pg_weighted_some prob=pg weighted=some
s_mixed_weighted prob=mixed weighted=some
s_builtin_weighted_force prob=builtin weighted=some force=1
s_builtin_force prob=builtin force=1
s_pg_force prob=pg force=1
s_builtin_cb prob=builtin cb=count
s_moved_force prob=moved force=1
s_moved_cb prob=moved cb=count
s_bound_cb prob=bound cb=count
s_builtin_force_iter_subset prob=builtin force=1 ls=iterative_schur pc=subset
s_builtin_cb_abort prob=builtin cb=abort
s_builtin_cb_success prob=builtin cb=success
s_builtin_cb_state prob=builtin cb=state
s_moved_iter prob=moved ls=iterative_schur
s_builtin_otherchart prob=builtin chart=other
s_builtin_userchart prob=builtin chart=user
s_builtin_bounded prob=builtin bounded=1
s_builtin_extra prob=builtin extra=1
s_scaled_otherchart prob=scaled chart=other
s_pg_nochart prob=pg chart=none
s_pg_bounded prob=pg bounded=1
s_pg_gaugefree prob=pg gaugefree=1
s_pg_iter prob=pg ls=iterative_schur pc=subset
s_bound_free prob=bound bounded=0
s_empty prob=empty
s_big prob=big
s_builtin_maxit0 prob=builtin maxit=0
c_builtin kind=cov prob=builtin
c_builtin_nopairs kind=cov prob=builtin pairs=none
c_builtin_foreign kind=cov prob=builtin pairs=self+foreign
c_builtin_extra kind=cov prob=builtin pairs=self+extra extra=1
c_builtin_nsr kind=cov prob=builtin nsr=1
c_user kind=cov prob=user
c_scaled kind=cov prob=scaled
c_pg kind=cov prob=pg
c_pg_nopairs kind=cov prob=pg pairs=none
c_pg_foreign kind=cov prob=pg pairs=self+foreign
c_pg_extra kind=cov prob=pg pairs=self+extra extra=1
c_bound kind=cov prob=bound
c_bound_extra kind=cov prob=bound pairs=self+extra extra=1
c_builtin_campt_cross0 kind=cov prob=builtin pairs=campt cross=0
c_builtin_ptpt_cross0 kind=cov prob=builtin pairs=ptpt cross=0
c_builtin_self_campt_ptpt_cross1 kind=cov prob=builtin pairs=self+campt+ptpt cross=1
c_builtin_extra_cross kind=cov prob=builtin pairs=extra extra=1 cross=1
c_builtin_prior kind=cov prob=builtin prior=1
c_builtin_rel kind=cov prob=builtin rel=1
c_builtin_otherchart kind=cov prob=builtin chart=other
c_builtin_userchart kind=cov prob=builtin chart=user
c_user_self_campt_ptpt_cross1 kind=cov prob=user pairs=self+campt+ptpt cross=1
c_scaled_self_campt_ptpt_cross1 kind=cov prob=scaled pairs=self+campt+ptpt cross=1
c_scaled_prior kind=cov prob=scaled prior=1
c_builtin_prior_rel kind=cov prob=builtin prior=w rel=w
c_builtin_weighted kind=cov prob=builtin weighted=some
c_builtin_bounded kind=cov prob=builtin bounded=1
c_builtin_constpt kind=cov prob=builtin constpt=1 pairs=ptpt cross=1
c_builtin_loss_huber_optin0 kind=cov prob=builtin loss=huber ba_losses=0
c_builtin_loss_huber_optin1 kind=cov prob=builtin loss=huber ba_losses=1
c_builtin_loss_unknown_optin1 kind=cov prob=builtin loss=unknown ba_losses=1
c_scaled_loss_huber_optin1 kind=cov prob=scaled loss=huber ba_losses=1
c_pg_loss_huber_optin0 kind=cov prob=pg loss=huber ba_losses=0
c_pg_loss_unknown_optin0 kind=cov prob=pg loss=unknown ba_losses=0
c_bound_loss_huber_optin0 kind=cov prob=bound loss=huber ba_losses=0
c_builtin_loss_some_optin kind=cov prob=builtin loss=scaled loss_on=some ba_losses=1 weighted=some
c_builtin_loss_noapply kind=cov prob=builtin loss=huber ba_losses=1 apply=0
c_builtin_prior_loss_optin kind=cov prob=builtin prior=loss ba_losses=1
c_builtin_loss_nsr kind=cov prob=builtin loss=unknown nsr=1
c_pg_loss_some kind=cov prob=pg loss=scaled loss_on=some
c_pg_loss_noapply kind=cov prob=pg loss=huber apply=0
c_pg_weighted kind=cov prob=pg weighted=some
c_pg_gaugefree kind=cov prob=pg gaugefree=1
c_pg_gaugefree_nopairs kind=cov prob=pg gaugefree=1 pairs=none
s_builtin_loss_badhuber prob=builtin loss=badhuber ba_losses=1
c_builtin_loss_badhuber kind=cov prob=builtin loss=badhuber ba_losses=1
s_builtin_weighted_nan prob=builtin weighted=nan
c_builtin_weighted_nan kind=cov prob=builtin weighted=nan
s_pg_loss_badhuber prob=pg loss=badhuber ba_losses=1
c_pg_loss_badhuber kind=cov prob=pg loss=badhuber ba_losses=1
s_pg_weighted_nan prob=pg weighted=nan
c_pg_weighted_nan kind=cov prob=pg weighted=nan
c_builtin_gaugefree kind=cov prob=builtin gaugefree=1
c_builtin_failjac kind=cov prob=builtin chart=failjac
c_scaled_failjac kind=cov prob=scaled chart=failjac
c_empty kind=cov prob=empty
c_big kind=cov prob=big
"""


def cases():
    return CASES.strip().splitlines()


def build_driver(out, include_dir=None, extra_flags=()):
    """g++ the driver against an include directory (the tree's by default) and the tree's libstba.so"""
    import importlib
    st = importlib.import_module("slam-tricks_amd")
    if not os.path.exists(st.LIB_PATH):
        importlib.import_module("slam-tricks_amd.build").build()
    pkg = os.path.join(ROOT, "slam-tricks_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", *extra_flags, "-I", include_dir or os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "ceres_routes_driver.cpp"), "-L", pkg, "-lstba", f"-Wl,-rpath,{pkg}", "-o", out])
    return out


def run_driver(exe, workdir, env=None):
    """every case through one process -> {name: {field: text, ..., "stderr": text}}"""
    listing = os.path.join(str(workdir), "cases.txt")
    with open(listing, "w") as f:
        f.write("\n".join(cases()) + "\n")
    p = subprocess.run([exe, listing], capture_output=True, text=True, timeout=600, env=env)
    assert p.returncode == 0, p.stderr[-4000:]
    return parse(p.stdout, p.stderr)


def parse(stdout, stderr):
    got = {}
    for line in stdout.splitlines():
        name, *rest = line.split("\t")
        assert len(rest) == len(FIELDS) - 1, line
        got[name] = dict(zip(FIELDS, rest))
    for chunk in stderr.split("@@ ")[1:]:
        name, _, text = chunk.partition("\n")
        got[name]["stderr"] = text
    assert list(got) == [c.split()[0] for c in cases()]
    return got


def golden(which):
    """{name: [the FIELDS]} -> {name: {field: text}}.  stderr is stored as "=" where it is the message and a newline (Solve's
    refusals) and as "C" where it is that behind "stba_ceres::Covariance: " (a Compute that failed)"""
    with open(os.path.join(ROOT, "tests", "golden", f"ceres_routes_{which}.json")) as f:
        out = {name: dict(zip(FIELDS, row)) for name, row in json.load(f).items()}
    for rec in out.values():
        rec["stderr"] = {"=": rec["message"] + "\n", "C": "stba_ceres::Covariance: " + rec["message"] + "\n"}.get(rec["stderr"], rec["stderr"])
    return out


def compare(got, want, bitwise):
    """strings exactly; Evaluate counts at most the recorded ones; with `bitwise` (same device library, same call sequence) the
    iteration counts and the costs in every bit"""
    assert list(got) == list(want)
    bad = []
    for name, w in want.items():
        g = got[name]
        for k in ("term", "path", "kept", "callbacks", "extra", "message", "stderr"):
            if g[k] != w[k]:
                bad.append(f"{name}: {k}: {g[k]!r} != {w[k]!r}")
        if int(g["evals"]) > int(w["evals"]):
            bad.append(f"{name}: evals {g['evals']} > {w['evals']}")
        if bitwise and (g["iters"], g["cost"]) != (w["iters"], w["cost"]):
            bad.append(f"{name}: iters/cost {g['iters']} {g['cost']} != {w['iters']} {w['cost']}")
    assert not bad, "\n".join(bad)
