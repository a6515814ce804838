// Stand-alone driver of slam-tricks_amd/csrc/inner_plan.hpp for tests/test_inner_plan_cpu.py: no device, no HIP.
// One case on stdin, whitespace-separated integers:
//   <nc> <np> <no>
//   <has cam_fixed_mask> [<nc masks, bit a = dof a constant>]     <has pt_fixed> [<np flags>]
//   <has rot_group> [<nc ids>]     <has pos_group> [<nc ids>]     <has pt_group> [<np ids>]
//   <no obs_cam> <no obs_pt>
// A "has" of 0 passes a null pointer.  stdout: "error: <why>", or the plan:
//   groups <n>
//   range <cam_lo> <cam_hi> <pt_lo> <pt_hi>        (n lines, ascending group id)
//   cam ... | pt ... | mask ... | kind ...         (four lines)
#include <cstdio>
#include <iostream>
#include <string>
#include <vector>

#include "../../slam-tricks_amd/csrc/inner_plan.hpp"

// <has> [<n values>] -> the values, *has says whether the pointer is passed
template <class T>
static std::vector<T> get_optional(int n, bool* has) {
    int h = 0;
    std::cin >> h;
    *has = h != 0;
    std::vector<T> v((size_t)(*has ? n : 0));
    for (auto& x : v) { int t = 0; std::cin >> t; x = (T)t; }
    return v;
}

template <class T>
static void put_list(const char* name, const std::vector<T>& v) {
    printf("%s", name);
    for (const T x : v) printf(" %d", (int)x);
    printf("\n");
}

int main() {
    int nc = 0, np = 0, no = 0;
    std::cin >> nc >> np >> no;
    bool has_cf = false, has_pf = false, has_rot = false, has_pos = false, has_pt = false;
    const std::vector<unsigned char> cf = get_optional<unsigned char>(nc, &has_cf), pf = get_optional<unsigned char>(np, &has_pf);
    const std::vector<int> rot = get_optional<int>(nc, &has_rot), pos = get_optional<int>(nc, &has_pos), pt = get_optional<int>(np, &has_pt);
    std::vector<int> oc((size_t)no), op((size_t)no);
    for (auto& x : oc) std::cin >> x;
    for (auto& x : op) std::cin >> x;
    if (!std::cin) { fprintf(stderr, "short or malformed case\n"); return 2; }
    stba::InnerPlan plan;
    std::string why;
    if (stba::build_inner_plan(nc, np, no, oc.data(), op.data(), has_cf ? cf.data() : nullptr, has_pf ? pf.data() : nullptr,
                               has_rot ? rot.data() : nullptr, has_pos ? pos.data() : nullptr, has_pt ? pt.data() : nullptr, &plan, &why) != 0) {
        printf("error: %s\n", why.c_str());
        return 0;
    }
    printf("groups %zu\n", plan.groups.size());
    for (const stba::InnerGroup& g : plan.groups) printf("range %d %d %d %d\n", g.cam_lo, g.cam_hi, g.pt_lo, g.pt_hi);
    put_list("cam", plan.cam); put_list("pt", plan.pt); put_list("mask", plan.mask); put_list("kind", plan.kind);
    return 0;
}
