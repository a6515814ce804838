"""The cases of tests/test_pg_plan_cpu.py and the command lines tests/cpp/pg_plan_driver.cpp reads them from.  CPU only, numpy.

Every graph case is (n, edge_i, edge_j, group_opt, limits): limits is a list of (one_kernel_solve, several_ranks, cus, lds_max_optin)
for pg_one_kernel_fits.  The boundary sizes are worked out from the formulas of slam-tricks_amd/csrc/pg_plan.hpp, restated in
tests/pg_plan_ref.py (which the test holds against the header's own constants)."""
import itertools

import numpy as np

import pg_plan_ref as R

ROOMY = (1, 0, 1000, 160 * 1024)          # one rank, more compute units and LDS than any plan here needs


def chain(n):
    return list(range(n - 1)), list(range(1, n))


def chain_with_closures(n=37):
    ei, ej = chain(n)
    for a, b in ((0, 36), (30, 3), (5, 20), (20, 5), (36, 18), (7, 8)):      # both directions, and a second edge beside an odometry edge
        ei.append(a); ej.append(b)
    return ei, ej


def star(n=23, hub=9):
    """every other node to the hub, alternating direction, then the hub's neighbours once more"""
    ei, ej = [], []
    for k in range(n):
        if k != hub:
            ei.append(hub if k % 2 else k); ej.append(k if k % 2 else hub)
    for k in (hub - 1, hub + 1):
        ei.append(k); ej.append(hub)
    return ei, ej


def parallel(count):
    """`count` edges between nodes 0 and 1, in both directions"""
    return [k % 2 for k in range(count)], [1 - k % 2 for k in range(count)]


def _graphs():
    g = {}

    def add(name, n, edges, group_opt=0, limits=(ROOMY,)):
        g[name] = dict(n=n, ei=list(edges[0]), ej=list(edges[1]), group_opt=group_opt, limits=list(limits))

    add("two_nodes", 2, ([0], [1]))
    add("two_nodes_reversed", 2, ([1], [0]))
    add("first_node_bare", 5, ([1, 2, 3], [2, 3, 4]), 2)
    add("middle_node_bare", 5, ([0, 1, 3], [1, 4, 4]), 2)
    add("last_node_bare", 5, ([0, 1, 2], [1, 2, 3]), 2)
    add("parallel_both_directions", 3, ([0, 1, 0, 2, 1, 0], [1, 0, 1, 1, 2, 1]), 2)
    for grp in (0, 2, 4, 8, 16, 32, 64):
        add(f"chain37_group{grp}", 37, chain_with_closures(), grp)
    add("star", 23, star(), 4)
    # ---- automatic group size: 8 while there are at most 200 groups
    add("auto_1600_keeps_8", 1600, chain(1600))
    add("auto_1601_doubles", 1601, chain(1601))
    add("auto_3201_doubles_twice", 3201, chain(3201))
    # ---- group_opt
    add("off", 37, chain_with_closures(), -1)
    for grp in (1, 3, 6):
        add(f"refused_group{grp}", 37, chain_with_closures(), grp)
    add("one_group_larger_than_n", 37, chain_with_closures(), 64)
    add("one_group_2_to_20", 37, chain_with_closures(), 1 << 20)
    # ---- the build kernel's LDS: groups of two nodes on a chain
    n_fit = R.largest_chain_that_builds(2)
    add("build_lds_largest", n_fit, chain(n_fit), 2)
    add("build_lds_one_node_more", n_fit + 1, chain(n_fit + 1), 2)
    add("build_lds_one_group_more", n_fit + 2, chain(n_fit + 2), 2)
    # ---- one-kernel eligibility, a case on each side of every clause
    add("agg_64", 128, chain(128), 64)
    add("agg_128", 128, chain(128), 128)
    lds256 = R.pp_lds_bytes(256, 1536)
    add("na_256", 512, chain(512), 2, [ROOMY, (1, 0, 256, 160 * 1024), (1, 0, 255, 160 * 1024), (1, 0, 1000, lds256 + 64), (1, 0, 1000, lds256 + 56),
                                        (0, 0, 1000, 160 * 1024), (1, 1, 1000, 160 * 1024), (2, 0, 1000, 160 * 1024), (1, 0, 1000, 0), (1, 0, 1000, -5)])
    add("na_257", 514, chain(514), 2, [ROOMY, (1, 0, 257, 160 * 1024)])
    add("ends_at_vcap", 2, parallel(R.PP_VCAP // 2), 2)
    add("ends_above_vcap", 2, parallel(R.PP_VCAP // 2 + 1), 2)
    add("off_never_fits", 37, chain_with_closures(), -1)
    return g


GRAPHS = _graphs()

# a plan given as such, where no graph separates two clauses: (agg, na, nc, max_group_ends) + the limits
SYNTHETIC_FITS = {
    "na_257_alone": (2, 257, 1536, 4) + ROOMY,
    "nc_above_ncmax_alone": (2, 256, 1537, 4) + ROOMY,
    "nc_at_ncmax": (2, 256, 1536, 4) + ROOMY,
    "agg_0_unplanned": (0, 0, 0, 0) + ROOMY,
}

BAD_EDGES = {      # (n, ei, ej) -> the first bad edge
    "i_negative": (4, [0, -1, 2], [1, 2, 3]),
    "i_too_large": (4, [0, 1, 4], [1, 2, 3]),
    "j_negative": (4, [0, 1, 2], [1, -3, 3]),
    "j_too_large": (4, [0, 1, 2], [1, 2, 4]),
    "self_loop": (4, [0, 2, 2], [1, 2, 3]),
    "the_first_of_two": (4, [0, 1, 3, 9], [1, 2, 3, 0]),
    "edge_0": (4, [4, 1], [1, 2]),
}

_a, _b = chain(6)
_c, _d = list(range(6, 9)), list(range(7, 10))
GAUGE = {      # (n, ei, ej, fixed or None)
    "chain7_null": (7,) + chain(7) + (None,),
    "chain7_none_fixed": (7,) + chain(7) + ([0] * 7,),
    "chain7_node4_fixed": (7,) + chain(7) + ([0, 0, 0, 0, 1, 0, 0],),
    "second_component_free": (10, _a + _c, _b + _d, [1] + [0] * 9),
    "both_components_fixed": (10, _a + _c, _b + _d, [1] + [0] * 7 + [1, 0]),
    "bare_node_11": (11, _a + _c, _b + _d, [1] + [0] * 7 + [1, 0, 0]),
    # two gauge-free components, the one with the SMALLER smallest node is reported: {1, 4, 7} (3 nodes) before {2, 3, 5, 6, 8} (5)
    "two_free_components": (9, [7, 4, 8, 6, 5, 3], [4, 1, 6, 5, 3, 2], [1] + [0] * 8),
    "two_free_components_null": (9, [7, 4, 8, 6, 5, 3, 0], [4, 1, 6, 5, 3, 2, 1], None),
}


def _hex(x):
    return float(x).hex()


def eta_grid():
    """(forcing_eta0, forcing_eta_min, forcing_eta_final, function_tolerance, eta, g2, g2_new, cost_change, new_cost)"""
    ftol = 1e-6
    new_cost = 3.0
    edge = 100.0 * ftol * new_cost / (1.0 - 100.0 * ftol)          # cost_change ~ 100 ftol (new_cost + cost_change)
    changes = [0.0, 1e-9, float(np.nextafter(edge, 0)), edge, float(np.nextafter(edge, 1)), 0.5, -1e-3]
    # (edge and its two neighbours straddle the boundary of the final clamp; test_pg_plan_cpu.py checks that both sides occur)
    rows = []
    for eta0, eta_final, eta, g2, g2_new, change in itertools.product(
            (0.0, 0.1, 0.5), (0.0, 1e-3, 0.05), (0.1, 0.3, 0.34, 0.5), (0.0, 2.5), (0.0, 1e-4, 0.3, 2.4, 40.0, float("nan"), float("inf")), changes):
        rows.append((eta0, 0.01, eta_final, ftol, eta, g2, g2_new, change, new_cost))
    return rows


def waits_grid():
    """(coarse_async, coarse_async_after, coarse_async_decrease, forcing, jobs, iter, last_rel_decrease)"""
    return [(a, after, 0.5, forcing, jobs, it, dec) for a, after, forcing, jobs, it, dec in itertools.product(
        (0, 1, 2), (0, 1, 3), (0, 1), (0, 1, 2), (0, 1, 2, 3, 4), (0.0, 0.25, 0.5, float(np.nextafter(0.5, 1)), 0.98))]


def lines():
    """(the command lines, their keys): key = (kind, name or index)"""
    out, keys = ["constants"], [("constants", None)]
    for name, c in GRAPHS.items():
        lim = " ".join(str(v) for t in c["limits"] for v in t)
        out.append(f"graph {c['n']} {len(c['ei'])} {c['group_opt']} {len(c['limits'])} {lim} " + " ".join(map(str, c["ei"] + c["ej"])))
        keys.append(("graph", name))
    for name, (n, ei, ej) in BAD_EDGES.items():
        out.append(f"graph {n} {len(ei)} 0 0 " + " ".join(map(str, ei + ej)))
        keys.append(("bad", name))
    for name, t in SYNTHETIC_FITS.items():
        out.append("fits " + " ".join(map(str, t)))
        keys.append(("fits", name))
    for name, (n, ei, ej, fixed) in GAUGE.items():
        out.append(f"gauge {n} {len(ei)} {0 if fixed is None else 1} " + " ".join(map(str, list(ei) + list(ej) + (fixed or []))))
        keys.append(("gauge", name))
    for k, row in enumerate(eta_grid()):
        out.append("eta " + " ".join(_hex(v) for v in row))
        keys.append(("eta", k))
    for k, (a, after, d0, forcing, jobs, it, dec) in enumerate(waits_grid()):
        out.append(f"waits {a} {after} {_hex(d0)} {forcing} {jobs} {it} {_hex(dec)}")
        keys.append(("waits", k))
    return out, keys
