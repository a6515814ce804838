"""Reference for slam-tricks_amd/csrc/pg_plan.hpp, written from the definitions in the header's comments and not from its code:
numpy's stable argsort for the CSR of the edge ends, the sizing rules as formulas, a breadth-first search for the gauge, and the two
policies of the solve loop as the same sequence of double operations in Python floats.  CPU only, numpy."""
import math

import numpy as np

INVALID = -1                 # STBA_ERR_INVALID_ARGUMENT
PG_NPW = 128                 # nodes per workgroup of the node kernels
PP_VCAP = 1536               # edge ends of a group whose products fit the persistent kernel's LDS buffer
PP_NCMAX = 1536
PP_SLOT = 16
PP_GROUPS_MAX = 256
PP_GROUP_NODES_MAX = 64
PP_LDS_MAX = 160 * 1024 - 64
PG_COARSE_BUILD_LDS_MAX = 136 * 1024
WHY_POWER = "stba_pg_solve: coarse_group must be a power of two >= 2 (0: automatic, -1: off)"
WHY_LARGE = "stba_pg_solve: coarse space too large for this group size"


def pp_lds_bytes(na, nc):
    """doubles: rc, pts [nc] each | gat [na][PP_SLOT] | ul, rl [384] each | vbuf [PP_VCAP][6] | red [128] | 16"""
    return 8 * (2 * nc + na * PP_SLOT + 2 * 384 + PP_VCAP * 6 + 128 + 16)


def coarse_build_lds(nc, max_group_ends):
    """six coarse columns of doubles, four ints per edge end of the largest group"""
    return 6 * nc * 8 + 4 * max_group_ends * 4


def largest_chain_that_builds(agg):
    """the largest n whose chain 0 - 1 - ... - (n - 1), in groups of agg >= 2 nodes, still fits the build kernel's LDS (an inner group
    of a chain has 2 agg edge ends)"""
    na = (PG_COARSE_BUILD_LDS_MAX - 16 * 2 * agg) // (48 * 6)
    return na * agg


def ends(n, ei, ej):
    """the edge ends 2 e + side sorted by their node, stably: (node_start, end_code, end_node, end_pos, end_rem)"""
    ei, ej = np.asarray(ei, np.int64), np.asarray(ej, np.int64)
    node = np.stack([ei, ej], 1).reshape(-1)            # of end 2 e + side
    other = np.stack([ej, ei], 1).reshape(-1)
    order = np.argsort(node, kind="stable")
    pos = np.empty(len(order), np.int64)
    pos[order] = np.arange(len(order))
    node_start = np.concatenate([[0], np.cumsum(np.bincount(node, minlength=n))])
    return node_start, order, node[order], pos, other[order]


def plan(n, node_start, group_opt):
    """(rc, why, plan or None); plan: dict of agg, na, nc, np, parts, max_group_ends, build_lds_bytes"""
    agg = group_opt
    if agg == 0:
        agg = 8
        while -(-n // agg) > 200:
            agg *= 2
    off = dict(agg=-1, na=0, nc=0, np=0, parts=1, max_group_ends=0, build_lds_bytes=0)
    if agg < 0:
        return 0, "", off
    if agg < 2 or bin(agg).count("1") != 1:
        return INVALID, WHY_POWER, None
    na = -(-n // agg)
    nc = 6 * na
    bounds = np.minimum(np.arange(na + 1) * agg, n)
    max_ends = int(np.diff(np.asarray(node_start)[bounds]).max())
    if coarse_build_lds(nc, max_ends) > PG_COARSE_BUILD_LDS_MAX:
        return INVALID, WHY_LARGE, None
    return 0, "", dict(agg=agg, na=na, nc=nc, np=-(-nc // 128) * 128, parts=max(1, agg // PG_NPW), max_group_ends=max_ends,
                       build_lds_bytes=coarse_build_lds(nc, max_ends))


def fits(p, one_kernel_solve, several_ranks, cus, lds_max_optin):
    """one rank, a coarse space whose groups fit a workgroup (<= 64 nodes, <= PP_VCAP edge ends) and are all resident (one per compute
    unit, <= 256), the kernel's LDS within what it may ask for and within what the device lets a workgroup opt in to, less 64 bytes"""
    lds = pp_lds_bytes(p["na"], p["nc"])
    return int(one_kernel_solve != 0 and not several_ranks and 0 < p["agg"] <= PP_GROUP_NODES_MAX and p["na"] <= PP_GROUPS_MAX
               and p["nc"] <= PP_NCMAX and lds <= PP_LDS_MAX and p["na"] <= cus and lds <= max(0, lds_max_optin - 64)
               and p["max_group_ends"] <= PP_VCAP)


def first_bad_edge(n, ei, ej):
    for e, (a, b) in enumerate(zip(ei, ej)):
        if not (0 <= a < n and 0 <= b < n) or a == b:
            return e
    return -1


def gauge(n, ei, ej, fixed):
    """(ok, size, first_node): the component without a constant node that holds the smallest node index, by breadth-first search"""
    adj = [[] for _ in range(n)]
    for a, b in zip(ei, ej):
        adj[a].append(b); adj[b].append(a)
    seen = [False] * n
    for s in range(n):
        if seen[s]:
            continue
        comp, todo = [s], [s]
        seen[s] = True
        while todo:
            for v in adj[todo.pop()]:
                if not seen[v]:
                    seen[v] = True; comp.append(v); todo.append(v)
        if fixed is None or not any(fixed[v] for v in comp):
            return 0, len(comp), s
    return 1, -1, -1


def next_eta(eta0, eta_min, eta_final, ftol, eta, g2, g2_new, cost_change, new_cost):
    """Eisenstat & Walker's choice 2 with their safeguard, kept in [eta_min, eta0], then the clamp of the last steps.  max and min are
    spelled out as the C++ library defines them: std::max(a, b) = a < b ? b : a, std::min(a, b) = b < a ? b : a"""
    smax = lambda a, b: b if a < b else a
    smin = lambda a, b: b if b < a else a
    if not (eta0 > 0.0 and g2 > 0.0 and math.isfinite(g2_new)):
        return eta
    e2 = 0.9 * g2_new / g2
    if 0.9 * eta * eta > 0.1:
        e2 = smax(e2, 0.9 * eta * eta)
    eta = smin(eta0, smax(eta_min, e2))
    if eta_final > 0.0 and cost_change <= 100.0 * ftol * (new_cost + cost_change):
        eta = smax(eta_min, smin(eta, eta_final))
    return eta


def final_clamp_applies(ftol, cost_change, new_cost):
    return cost_change <= 100.0 * ftol * (new_cost + cost_change)


def waits_for_own_inverse(coarse_async, after, decrease, forcing, jobs, it, last_rel_decrease):
    """the first solve waits for its own inverse (coarse_async = 2 with a forcing sequence: not even that one), and -- unless
    coarse_async = 2 -- so does every solve of the first `after` iterations and every one behind a step that took more than
    `decrease` off the cost"""
    if jobs == 0 and not (forcing and coarse_async == 2):
        return 1
    if coarse_async == 2:
        return 0
    return int(it <= after or last_rel_decrease > decrease)
