// inner_plan.hpp -- the ordering of the BA engine's inner iterations (stba_ba_set_inner_iterations) as the sweep runs
// it: three group-id arrays, the constant masks and the observation list -> per-group ranges of a camera list (with each entry's dof
// mask) and a landmark list, in ascending group id.  Returns 0, or non-zero with the reason in *why.
// Host only: the standard library, nothing of HIP and nothing of include/stba.h (tests/cpp/inner_plan_driver.cpp).
#pragma once
#include <algorithm>
#include <cstddef>
#include <string>
#include <utility>
#include <vector>

namespace stba {

struct InnerGroup { int cam_lo, cam_hi, pt_lo, pt_hi; };
struct InnerPlan {
    std::vector<InnerGroup> groups;            // ascending group id
    std::vector<int> cam, pt;                  // camera list, landmark list
    std::vector<unsigned char> mask, kind;     // per camera entry: swept dofs; kind: 1 rotation, 2 position, 3 both (a 6-dof block)
};

// cam_fixed_mask [nc]: bit a = dof a constant; pt_fixed [np]; either may be null (nothing constant).  rot_group, pos_group [nc] and
// pt_group [np]: the group of every part, -1: not swept; a null array: none of its parts; all three null: the default ordering
// {cameras as 6-dof blocks}, {landmarks}.  The observations are read in the order given: a refusal names the first offending one.
// *out is written only on success
inline int build_inner_plan(int nc, int np, int no, const int* obs_cam, const int* obs_pt, const unsigned char* cam_fixed_mask,
                            const unsigned char* pt_fixed, const int* rot_group, const int* pos_group, const int* pt_group,
                            InnerPlan* out, std::string* why) {
    auto cf = [&](int c) { return cam_fixed_mask ? (unsigned)cam_fixed_mask[(size_t)c] : 0u; };
    const bool dflt = !rot_group && !pos_group && !pt_group;
    // group of every part (-1: not swept); constant parts are ignored
    std::vector<int> gr((size_t)nc, -1), gq((size_t)nc, -1), gp((size_t)np, -1);
    for (int c = 0; c < nc; ++c) {
        const bool rot_const = (cf(c) & 7u) == 7u, pos_const = (cf(c) & 56u) == 56u;
        const int r = dflt ? 0 : (rot_group ? rot_group[c] : -1), q = dflt ? 0 : (pos_group ? pos_group[c] : -1);
        if (r < -1 || q < -1) { *why = "camera " + std::to_string(c) + ": a group id below -1"; return 1; }
        gr[(size_t)c] = rot_const ? -1 : r;
        gq[(size_t)c] = pos_const ? -1 : q;
    }
    for (int j = 0; j < np; ++j) {
        const int g = dflt ? 1 : (pt_group ? pt_group[j] : -1);
        if (g < -1) { *why = "landmark " + std::to_string(j) + ": a group id below -1"; return 1; }
        gp[(size_t)j] = (pt_fixed && pt_fixed[(size_t)j]) ? -1 : g;
    }
    // independence: a residual touches one camera and one landmark, so a group is independent unless it holds a part of a camera and
    // a landmark that camera observes (a camera's rotation and position in one group are one 6-dof block)
    for (int i = 0; i < no; ++i) {
        const int c = obs_cam[(size_t)i], j = obs_pt[(size_t)i], g = gp[(size_t)j];
        if (g >= 0 && (g == gr[(size_t)c] || g == gq[(size_t)c])) {
            *why = "group " + std::to_string(g) + " is not an independent set: camera " + std::to_string(c) + " and landmark " + std::to_string(j) +
                   " share a residual";
            return 1;
        }
    }
    std::vector<int> ids;
    for (int c = 0; c < nc; ++c) { if (gr[(size_t)c] >= 0) ids.push_back(gr[(size_t)c]); if (gq[(size_t)c] >= 0) ids.push_back(gq[(size_t)c]); }
    for (int j = 0; j < np; ++j) if (gp[(size_t)j] >= 0) ids.push_back(gp[(size_t)j]);
    std::sort(ids.begin(), ids.end());
    ids.erase(std::unique(ids.begin(), ids.end()), ids.end());
    InnerPlan p;
    for (const int g : ids) {
        InnerGroup r;
        r.cam_lo = (int)p.cam.size(); r.pt_lo = (int)p.pt.size();
        for (int c = 0; c < nc; ++c) {
            const unsigned kind = (gr[(size_t)c] == g ? 1u : 0u) | (gq[(size_t)c] == g ? 2u : 0u);
            if (!kind) continue;
            const unsigned m = (((kind & 1u) ? 7u : 0u) | ((kind & 2u) ? 56u : 0u)) & ~cf(c);
            p.cam.push_back(c); p.mask.push_back((unsigned char)m); p.kind.push_back((unsigned char)kind);
        }
        for (int j = 0; j < np; ++j) if (gp[(size_t)j] == g) p.pt.push_back(j);
        r.cam_hi = (int)p.cam.size(); r.pt_hi = (int)p.pt.size();
        p.groups.push_back(r);
    }
    *out = std::move(p);
    return 0;
}

}  // namespace stba
